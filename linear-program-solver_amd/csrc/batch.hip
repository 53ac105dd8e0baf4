// Batched solve: many small LPs of one shape, one workgroup per LP, the LP's
// whole (m+1) x (n+1) float64 tableau in LDS for the life of a launch
// (lp_batch_* in include/lpgpu.h; DESIGN.md "Batched solve").
//
// The float semantics are the header comment of oracle/lp_f64.c, pivot for
// pivot; the solve logic is lpf_solve / lpf_run restated per LP.  There is no
// communication between workgroups and no waiting of any kind: a launch runs
// at most `chunk` pivots per LP, leaves each LP's state in a small global
// record, and the host relaunches while any LP is still in progress.
//
// The two-phase solve (lp_twophase_* in include/lpgpu.h) runs
// phase 1 per LP in the same way, on the tableau widened by its artificial
// columns; k_batch and k_twophase share one pivot iteration (bstep).
//
// A placed batch (lp_placed_* in include/lpgpu.h) may keep an LP
// that does not fit a CU's LDS in device memory for the whole launch:
// k_batch_dev runs the same bstep on the LP's global pointer, still one
// workgroup per LP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "batch_plan.h"
#include "device.h"
#include "knobs.h"

namespace lpk {
namespace {

constexpr int B_START = 0;    // the next launch begins a new lpf_solve / lpf_run
constexpr int B_RUNNING = 1;  // stopped at the launch's chunk bound
constexpr int B_DONE = 2;     // finished: later launches return at the top

// per-LP state between launches
struct BRec {
    int32_t status;   // lp_status of the finished call (LP_PIVOTED while running)
    int32_t state;    // B_*
    int32_t rule;     // rule in use (solve: standard until the stall switch)
    int32_t buf;      // k_batch_team: which of the LP's two tableau buffers is current (else 0, unused)
    long long npiv, nstd, stuck;
    double z0;        // objective at the start of the call
};

struct BArgs {
    double *T;          // count x (m+1) x (n+1), each LP contiguous
    BRec *rec;          // count
    long long *log;     // count x logcap x 2, or null
    int32_t *basis;     // count x m, or null
    long long count, logcap, chunk, limit;   // limit < 0: no cap
    int m, n, pitch;    // pitch: LDS row pitch in doubles (odd)
    int mode, run_rule;
    lp_tol tol;
};

// Ragged batches (lp_ragged_*): LPs of different shapes in one
// batch.  One entry per LP, written once at create; a ragged launch covers one
// bin of the plan (batch_plan.h) and takes each LP's shape from here.
struct BShape {
    long long toff;     // tableau: doubles from BArgs::T, LPs packed back to back
    long long boff;     // basis: entries from BArgs::basis (the m of the LPs before)
    long long woff;     // two-phase working tableau: doubles from TArgs::W, rows at n + 1 + m
    long long coff;     // two-phase saved costs: doubles from TArgs::origc
    int32_t m, n;
    int32_t pitch;      // the LP's own odd LDS pitch (n + 1) | 1 ...
    int32_t wpitch;     // ... and (n + 1 + m) | 1 for the widened two-phase layout
};

// what a ragged launch adds to BArgs / TArgs: block b of the launch solves LP
// order[b]; B.m, B.n, B.pitch are unused.  TArgs::ww is read by no launch,
// ragged or uniform: the kernels derive n + 1 + m themselves, the host still
// sets the field, and it stays because the argument layout is fixed
struct RBin {
    const BShape *shape;    // count
    const int32_t *order;   // this bin's LPs, ascending
    int nbin;               // = the grid
};
struct RArgs : BArgs {
    RBin R;
};

template <int WAVES>
__device__ __forceinline__ double bmin(double v, double *sc)
{
    if constexpr (WAVES == 1) return wave_min(v);
    else return block_min(v, sc);
}

template <int WAVES>
__device__ __forceinline__ long long bmin_ll(long long v, double *sc)
{
    if constexpr (WAVES == 1) return wave_min_ll(v);
    else return block_min_ll(v, reinterpret_cast<long long *>(sc));
}

// the counters of one lpf_solve / lpf_run in progress
struct BSolve {
    long long npiv, nstd, stuck;
    double z0;        // objective at the start of the call
    int rule;
};

// element e = i * w + j of the live (rows x w) tableau walked with a stride of
// NT threads, (i, j) carried along
struct BWalk {
    int w, E, di, dj, i0, j0;
};

template <int NT>
__device__ __forceinline__ BWalk bwalk(int rows, int w)
{
    const int tid = threadIdx.x;
    return BWalk{w, rows * w, NT / w, NT % w, tid / w, tid % w};
}

// f(e, i, j) for every element of the walk that this thread owns.  ONCE keeps
// the loop rolled (#pragma unroll 1), as the one-off stages of the two-phase
// kernels have it.
template <int NT, bool ONCE = false, class F>
__device__ __forceinline__ void walk(const BWalk &W, F f)
{
    int i = W.i0, j = W.j0;
    if constexpr (ONCE) {
#pragma unroll 1
        for (int e = threadIdx.x; e < W.E; e += NT) {
            f(e, i, j);
            j += W.dj;
            i += W.di;
            if (j >= W.w) { j -= W.w; ++i; }
        }
    } else {
        for (int e = threadIdx.x; e < W.E; e += NT) {
            f(e, i, j);
            j += W.dj;
            i += W.di;
            if (j >= W.w) { j -= W.w; ++i; }
        }
    }
}

// the counters of a call between launches: a new call's, the record's, and
// back to the record (thread 0 of the workgroup that owns it)
__device__ __forceinline__ BSolve solve_start(double z0, int rule)
{
    return BSolve{0, 0, 0, z0, rule};
}

__device__ __forceinline__ BSolve solve_load(const BRec *rp)
{
    return BSolve{rp->npiv, rp->nstd, rp->stuck, rp->z0, rp->rule};
}

// TEAM: k_batch_team's record also says which buffer is current
template <bool TEAM = false>
__device__ __forceinline__ void solve_store(BRec *rp, const BSolve &S, int status, bool done, int buf = 0)
{
    rp->status = status;
    rp->state = done ? B_DONE : B_RUNNING;
    rp->rule = S.rule;
    if constexpr (TEAM) rp->buf = buf;
    rp->npiv = S.npiv;
    rp->nstd = S.nstd;
    rp->stuck = S.stuck;
    rp->z0 = S.z0;
}

// lpf_pivot on tableau indices (R, C), a = T[R][C] != 0: save the multipliers
// and the normalised row, then one pass of FMAs over the whole live tableau
template <int NT>
__device__ __forceinline__ void bpivot(double *Tl, double *Pl, double *Fl, int m, int n, int pitch,
                                       const BWalk &W, long long R, long long C, double a)
{
    const int tid = threadIdx.x;
    for (int i = tid; i <= m; i += NT) Fl[i] = Tl[i * pitch + C];
    for (int j = tid; j <= n; j += NT) Pl[j] = j == C ? 1.0 : Tl[R * pitch + j] / a;
    __syncthreads();
    walk<NT>(W, [&](int, int i, int j) {
        const double x = Tl[i * pitch + j];
        Tl[i * pitch + j] = upd(i, R, Fl[i], Pl[j], x);
    });
    __syncthreads();
}

// ---------------------------------------------------------------------------
// Device-placed LPs (k_batch_dev): the tableau stays in device
// memory, contiguous at pitch n + 1; P, F and the scratch are in LDS.
// ---------------------------------------------------------------------------

// The flat walk of the LP's E = (m+1)(n+1) contiguous doubles in pairs, with a
// stride of NT pairs.  A pair is one aligned 16-byte access: `head` (0 or 1)
// elements are peeled at the front where the LP starts at an odd double (a
// ragged LP's toff, or an odd LP of an odd E), and one at the back where an
// odd count remains.  (i, j) of a thread's pair is carried along; the pair's
// second element is (i, j + 1) or, across a row end, (i + 1, 0).
struct DWalk {
    int w, E, head, di, dj, i0, j0;
};

template <int NT>
__device__ __forceinline__ DWalk dwalk(int rows, int w, int head)
{
    const int e0 = head + 2 * (int)threadIdx.x;
    return DWalk{w, rows * w, head, (2 * NT) / w, (2 * NT) % w, e0 / w, e0 % w};
}

// ---------------------------------------------------------------------------
// Teamed LPs (k_batch_team): a device-placed LP worked on by a
// team of workgroups, one launch per pivot.  Every workgroup of the team runs
// the whole selection on the LP's current buffer and then updates its own
// range [e0, e1) of the E elements out of place, into the LP's other buffer.
// ---------------------------------------------------------------------------

// DWalk restricted to one range.  Ranges end at pair boundaries of the buffer
// (batch_plan.h: plan_team_ranges), so `head` is 1 only for the range that
// starts an LP at an odd double and a tail element remains only where the LP
// ends inside a pair.  out: the LP in its other buffer; applied: whether this
// launch's pivot was written there (a zero pivot is counted, not applied).
struct TWalk {
    int w, e0, e1, head, di, dj, i0, j0;
    double *out;
    mutable bool applied;
};

template <int NT>
__device__ __forceinline__ TWalk twalk(int w, int e0, int e1, int head, double *out)
{
    const int e = e0 + head + 2 * (int)threadIdx.x;
    return TWalk{w, e0, e1, head, (2 * NT) / w, (2 * NT) % w, e / w, e % w, out, false};
}

// lpf_pivot on a device-placed LP: one pass of 16-byte accesses over the walk's
// range, read from Tin.  F[1..m] was staged by the ratio test.
//
// DWalk (k_batch_dev, k_twophase_dev): the whole LP, [0, E), updated in place.
// Visibility: the only producer and consumer of this LP's bytes within a
// launch is this workgroup, on one CU, so __syncthreads()'s workgroup-scope
// release / acquire is what orders these stores before the next selection's
// loads; no agent-scope fence, no cache-bypassing access, and the kernel
// boundary orders the launches.
//
// TWalk (k_batch_team): one workgroup's range [e0, e1), written to W.out.
// Visibility: within a launch no workgroup reads a word that another workgroup
// writes -- the selection and this pass read only the LP's current buffer and
// the input records, every store of a launch goes to the other buffer, the
// output records, the log or the basis, and none of those is read before the
// next launch.  The kernel boundary on the batch's one stream is the only
// ordering there is: no fence, no cache-bypassing access, no atomic, no flag,
// no cooperative launch, and no loop that is not bounded by an argument.
// the range a walk covers and where its updated elements go: the whole LP in
// place (DWalk), or [e0, e1) into the other buffer (TWalk).  Overloads, not
// locals set under `if constexpr` in bpivot_dev: with locals the compiler
// emitted 40 to 130 more lines for every kernel that uses the pass, with
// these the bodies are the ones the two separate functions compiled to.
__device__ __forceinline__ int wbeg(const DWalk &) { return 0; }
__device__ __forceinline__ int wbeg(const TWalk &W) { return W.e0; }
__device__ __forceinline__ int wend(const DWalk &W) { return W.E; }
__device__ __forceinline__ int wend(const TWalk &W) { return W.e1; }
__device__ __forceinline__ double *wout(const DWalk &, const double *T) { return const_cast<double *>(T); }
__device__ __forceinline__ double *wout(const TWalk &W, const double *) { return W.out; }

template <int NT, class WALK>
__device__ __forceinline__ void bpivot_dev(const double *Tin, double *Pl, double *Fl, int n, const WALK &W,
                                           long long R, long long C, double a)
{
    constexpr bool TEAM = std::is_same_v<WALK, TWalk>;
    const int tid = threadIdx.x;
    if (tid == 0) Fl[0] = Tin[C];
    for (int j = tid; j <= n; j += NT) Pl[j] = j == C ? 1.0 : Tin[R * W.w + j] / a;
    __syncthreads();
    double *const To = wout(W, Tin);
    int i = W.i0, j = W.j0;
#pragma unroll 4
    for (int e = wbeg(W) + W.head + 2 * tid; e + 1 < wend(W); e += 2 * NT) {
        double2 x = *reinterpret_cast<const double2 *>(Tin + e);
        int i1 = i, j1 = j + 1;
        if (j1 >= W.w) { j1 = 0; ++i1; }
        x.x = upd(i, R, Fl[i], Pl[j], x.x);
        x.y = upd(i1, R, Fl[i1], Pl[j1], x.y);
        *reinterpret_cast<double2 *>(To + e) = x;
        j += W.dj;
        i += W.di;
        if (j >= W.w) { j -= W.w; ++i; }
    }
    // the peeled ends: a head is element 0 = (0, 0), a tail the range's last
    // element -- (m, n) where the range is the whole LP
    if (tid == 0 && W.head) To[wbeg(W)] = upd(0, R, Fl[0], Pl[0], Tin[wbeg(W)]);
    if (tid == NT - 1 && ((wend(W) - wbeg(W) - W.head) & 1)) {
        // in place the last element is known to be (m, n) = (E / w - 1, n): one
        // divide and no remainder; a team's range ends anywhere, so el / w, el % w
        const int el = wend(W) - 1, il = TEAM ? el / W.w : wend(W) / W.w - 1, jl = TEAM ? el % W.w : n;
        To[el] = upd(il, R, Fl[il], Pl[jl], Tin[el]);
    }
    if constexpr (TEAM) W.applied = true;
    else __syncthreads();
}

// row i's entry of column C for the first loop of the ratio test; a
// device-placed LP stages it into F on the way
template <bool DEV>
__device__ __forceinline__ double ratio_a(double *Tl, double *Fl, int i, int pitch, long long C)
{
    if constexpr (DEV) return Fl[i] = Tl[i * pitch + C];
    else return Tl[i * pitch + C];
}

// The entering column of lpf_find_max_increase (LP_RULE_MAX_INCREASE; DESIGN.md
// 4n): lanes across columns, each lane walking its whole column in row order.
// In LDS the lanes of a wave read Tl[i * pitch + j] at consecutive addresses
// and b_i is a broadcast; in device memory (DEV) the same reads are coalesced
// whatever the LP's first double, and column 0 comes from the cache.  A column
// takes part iff c_j < -tol.cost; g_j is lpf_min_ratio (from +inf, q taken iff
// q < g_j, so a NaN or +inf ratio never is); the divide is skipped for rows
// that are not eligible and for columns that do not take part.  inc_j (-inf
// for a column that does not take part, as the oracle's array) goes to P[j],
// which is dead between pivots; the thread that writes P[j] is the one that
// reads it back below.  Returns true when the LP ends here (status set); else
// k is this thread's first column inside the band of the largest increase, or
// NONE.  Every exit is taken from block-reduced values.
template <int WAVES>
__device__ __forceinline__ bool bmaxinc(const double *Tl, double *Pl, double *sc, int m, int n, int pitch,
                                        const lp_tol &tol, long long &k, int &status)
{
    constexpr int NT = 64 * WAVES;
    const int tid = threadIdx.x;
    long long f = NONE;     // 0: a column that takes part has no finite ratio; 1: some column takes part
    double v = INFINITY;    // min -inc_j: the maximum under inc > M, a NaN never taken
    for (int j = 1 + tid; j <= n; j += NT) {
        const double c = Tl[j];
        double inc = -INFINITY;
        if (c < -tol.cost) {
            double g = INFINITY;
#pragma unroll 4
            for (int i = 1; i <= m; ++i) {
                const double a = Tl[i * pitch + j];
                const double b = Tl[i * pitch];
                if (a > tol.pivot) {
                    const double q = (fabs(b) <= tol.zero ? 0.0 : b) / a;
                    if (q < g) g = q;
                }
            }
            if (!(g < INFINITY)) f = 0;
            else if (f == NONE) f = 1;
            inc = -c * g;
            v = fmin(v, -inc);
        }
        Pl[j] = inc;
    }
    f = bmin_ll<WAVES>(f, sc);
    if (f == NONE) {
        status = LP_OPTIMAL;
        return true;
    }
    if (f == 0) {                       // whatever the other columns hold
        status = LP_UNBOUNDED;
        return true;
    }
    const double M = -bmin<WAVES>(v, sc);
    const double thr = M - tol.ratio_tie * fabs(M);
    for (int j = 1 + tid; j <= n; j += NT)
        if (Pl[j] >= thr && k == NONE) k = j;
    return false;
}

// The start of a call under LP_RULE_DUAL: true where some cost
// T[0][j] < -tol.cost, j = 1..n -- the LP is not dual feasible and the rule is
// not defined on it.  Block-reduced: every thread gets the same answer.
template <int WAVES>
__device__ __forceinline__ bool bdual_start(const double *Tl, double *sc, int n, const lp_tol &tol)
{
    constexpr int NT = 64 * WAVES;
    long long f = NONE;
    for (int j = 1 + (int)threadIdx.x; j <= n; j += NT)
        if (Tl[j] < -tol.cost) f = 0;
    return bmin_ll<WAVES>(f, sc) != NONE;
}

// The selection of one dual simplex step (LP_RULE_DUAL), next to
// bmaxinc: the leaving row first, lanes over rows of column 0 as the ratio test
// walks them; then the entering column, lanes over the columns of row R and of
// row 0 (consecutive addresses in LDS and in device memory alike).  Row i takes
// part iff b_i < -tol.zero; R is the first such row inside the band of their
// exact minimum.  Column j takes part iff a = T[R][j] < -tol.pivot; its ratio is
// (|c_j| <= tol.cost ? 0 : c_j) / -a, and C is the first such column inside the
// band of the exact minimum ratio (fmin: a NaN ratio is never the minimum, and
// never inside a band).  Both argmins are two-pass, so neither depends on the
// reduction order.  Returns true when the LP ends here (status set), with no
// pivot applied: no row takes part (LP_OPTIMAL), no column does (LP_INFEASIBLE:
// row R proves it), or a band that is NaN holds nothing (LP_BAD_PIVOT).  Every
// exit is taken from block-reduced values.  DEV: column C is staged into
// F[1..m] once it is known, where bpivot_dev expects it (the ratio test's first
// loop does that for the primal rules).
template <int WAVES, bool DEV>
__device__ __forceinline__ bool bdual(const double *Tl, double *Fl, double *sc, int m, int n, int pitch,
                                      const lp_tol &tol, long long &R, long long &C, int &status)
{
    constexpr int NT = 64 * WAVES;
    const int tid = threadIdx.x;
    double v = INFINITY;
    for (int i = 1 + tid; i <= m; i += NT) {
        const double b = Tl[i * pitch];
        if (b < -tol.zero) v = fmin(v, b);
    }
    double g = bmin<WAVES>(v, sc);
    if (!(g < INFINITY)) {              // no row takes part: +inf is not below -tol.zero
        status = LP_OPTIMAL;
        return true;
    }
    double thr = g + tol.cost_tie * fabs(g);
    long long k = NONE;
    for (int i = 1 + tid; i <= m; i += NT) {
        const double b = Tl[i * pitch];
        if (b < -tol.zero && b <= thr && k == NONE) k = i;
    }
    R = bmin_ll<WAVES>(k, sc);
    if (R == NONE) {                    // b = -inf: the band is NaN
        status = LP_BAD_PIVOT;
        return true;
    }
    const double *const row = Tl + R * pitch;
    long long f = NONE;
    v = INFINITY;
    for (int j = 1 + tid; j <= n; j += NT) {
        const double a = row[j];
        if (a < -tol.pivot) {
            const double c = Tl[j];
            v = fmin(v, (fabs(c) <= tol.cost ? 0.0 : c) / -a);
            f = 0;
        }
    }
    f = bmin_ll<WAVES>(f, sc);
    if (f == NONE) {
        status = LP_INFEASIBLE;
        return true;
    }
    g = bmin<WAVES>(v, sc);
    thr = g + tol.ratio_tie * fabs(g);
    k = NONE;
    for (int j = 1 + tid; j <= n; j += NT) {
        const double a = row[j];
        if (a < -tol.pivot) {
            const double c = Tl[j];
            if ((fabs(c) <= tol.cost ? 0.0 : c) / -a <= thr && k == NONE) k = j;
        }
    }
    C = bmin_ll<WAVES>(k, sc);
    if (C == NONE) {                    // only NaN ratios
        status = LP_BAD_PIVOT;
        return true;
    }
    if constexpr (DEV)
        for (int i = 1 + tid; i <= m; i += NT) Fl[i] = Tl[i * pitch + C];
    return false;
}

// One iteration of lpf_solve / lpf_run on the live m x n tableau in LDS, shared
// by k_batch and k_twophase.  Returns true when the call ends (status set).
// Every exit is taken from block-reduced or LDS-resident values that all
// threads read identically, so the barriers inside stay uniform.  basis / log
// are this LP's (null: none kept); logroom = log entries left for this call.
//
// DEV (k_batch_dev): Tl is the LP's tableau in device memory at
// pitch n + 1 and W the walk of bpivot_dev.  Every decision is the same code;
// what differs is that the first loop of the ratio test stages column C into
// F (so the strided column is read from memory once, not three times) and
// that the update is bpivot_dev's walk.
//
// TEAM (k_batch_team): DEV with Tl the LP's current buffer, read
// only; the update is bpivot_dev over the team's range into the other buffer, and the new
// T[0][0] the stall test needs is computed here, by every workgroup of the
// team alike, as the fma its owner stores.
//
// MAXINC (LP_RULE_MAX_INCREASE): the entering column is
// bmaxinc's; the ratio test, the pivot, the basis and the log are the same
// code.  Only lp_batch_run asks for it (MODE_RUN), through instantiations of
// their own, so the others compile to what they compiled to without it.
//
// DUAL (LP_RULE_DUAL): the whole selection is bdual's, leaving row
// first; the pivot, the basis and the log are the same code.  Reached as MAXINC
// is, through instantiations of its own.
template <int WAVES, bool DEV = false, typename WALK = BWalk, bool TEAM = false, bool MAXINC = false,
          bool DUAL = false>
__device__ __forceinline__ bool bstep(double *Tl, double *Pl, double *Fl, double *sc, int m, int n,
                                      int pitch, const WALK &W, const lp_tol &tol, int mode,
                                      long long limit, BSolve &S, int &status, int32_t *basis,
                                      long long *log, long long logroom)
{
    constexpr int NT = 64 * WAVES;
    const int tid = threadIdx.x;
    if (mode == MODE_SOLVE && S.rule == LP_RULE_STANDARD && S.stuck >= (long long)m + n)
        S.rule = LP_RULE_MIN_INDEX;
    if (limit >= 0 && S.npiv >= limit) {      // before the selection, as lpf_solve
        status = mode == MODE_SOLVE ? LP_CAP_REACHED : LP_PIVOTED;
        return true;
    }

    long long R, C;
    if constexpr (DUAL) {
        if (bdual<WAVES, DEV>(Tl, Fl, sc, m, n, pitch, tol, R, C, status)) return true;
    } else {
        // ---- entering column (entering() in lp_f64.c)
        long long k = NONE;
        if constexpr (MAXINC) {
            if (bmaxinc<WAVES>(Tl, Pl, sc, m, n, pitch, tol, k, status)) return true;
        } else if (S.rule == LP_RULE_MIN_INDEX) {
            for (int j = 1 + tid; j <= n; j += NT)
                if (Tl[j] < -tol.cost && k == NONE) k = j;
        } else {
            double v = INFINITY;
            for (int j = 1 + tid; j <= n; j += NT) v = fmin(v, Tl[j]);
            const double g = bmin<WAVES>(v, sc);
            if (g < -tol.cost) {
                const double thr = g + tol.cost_tie * fabs(g);
                for (int j = 1 + tid; j <= n; j += NT)
                    if (Tl[j] <= thr && k == NONE) k = j;
            }
        }
        C = bmin_ll<WAVES>(k, sc);
        if (C == NONE) {                    // MAXINC: lpf_find_max_increase's c = -1 (a NaN band)
            status = MAXINC ? LP_BAD_PIVOT : LP_OPTIMAL;
            return true;
        }

        // ---- ratio test (leaving() in lp_f64.c): eligibility is a flag, the
        // minimum starts at the first eligible row's ratio (a NaN there stays),
        // the band g + tie |g| is not clamped
        double v = INFINITY;
        long long fe = NONE;
        for (int i = 1 + tid; i <= m; i += NT) {
            bool ok;
            const double q = row_ratio(ratio_a<DEV>(Tl, Fl, i, pitch, C), Tl[i * pitch], tol, ok);
            if (ok) {
                v = fmin(v, q);
                if (fe == NONE) fe = 2LL * i + (q != q ? 1 : 0);
            }
        }
        double g = bmin<WAVES>(v, sc);
        fe = bmin_ll<WAVES>(fe, sc);
        if (fe == NONE) {
            status = LP_UNBOUNDED;
            return true;
        }
        if (fe & 1) g = NAN;
        const double thr = g + tol.ratio_tie * fabs(g);
        k = NONE;
        for (int i = 1 + tid; i <= m; i += NT) {
            bool ok;
            const double q = row_ratio(DEV ? Fl[i] : Tl[i * pitch + C], Tl[i * pitch], tol, ok);
            if (ok && q <= thr && k == NONE) k = i;
        }
        R = bmin_ll<WAVES>(k, sc);
        if (R == NONE) {                    // lp_f64.c's "unreachable" -1 (a NaN band)
            status = LP_UNBOUNDED;
            return true;
        }
    }

    // ---- pivot (lpf_pivot)
    const double a = Tl[R * pitch + C];
    if (a != 0.0) {                     // lpf_solve counts a zero pivot without applying it
        if constexpr (DEV) bpivot_dev<NT>(Tl, Pl, Fl, n, W, R, C, a);
        else bpivot<NT>(Tl, Pl, Fl, m, n, pitch, W, R, C, a);
    }
    if (tid == 0) {
        if (basis) basis[R - 1] = (int32_t)(C - 1);
        if (S.npiv < logroom) {
            long long *const l = log + S.npiv * 2;
            l[0] = R - 1;
            l[1] = C - 1;
        }
    }
    ++S.npiv;
    if (mode == MODE_SOLVE && S.rule == LP_RULE_STANDARD) {
        ++S.nstd;
        double z;
        if constexpr (TEAM) z = -(a != 0.0 ? upd(0, R, Fl[0], Pl[0], Tl[0]) : Tl[0]);
        else z = -Tl[0];
        const double band = tol.stall * fmax(1.0, fabs(S.z0));
        if (z - S.z0 > band) {
            status = LP_OBJ_INCREASED;  // after the offending pivot
            return true;
        }
        if (fabs(z - S.z0) <= band) ++S.stuck;
        else S.stuck = 0;
    }
    return false;
}

// LDS: tableau rows at `pitch` doubles (odd: the ratio test reads a column,
// lanes over rows, 2*pitch dwords apart -- distinct banks mod 64 per 32-lane
// half), then the normalised pivot row P (pitch), the multipliers F (m+1) and
// the reduction scratch (16).
// a value every thread of the block holds identically, moved to a scalar
// register so that the branches on it are scalar branches
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni(long long v)
{
    const unsigned lo = (unsigned)uni((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)uni((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---- the per-LP prologue of every solve kernel.  RAGGED: the launch is one
// bin of a ragged batch's plan -- the LP comes from the bin's order array and
// its shape, pitch and base offsets from the LP's table entry; below these
// two helpers the two forms are one code.  Everything read from a table comes
// back through uni(): every thread of the block holds it identically.

// the LP this workgroup solves, or -1: the block is beyond the launch's LPs
template <bool RAGGED, class ARGS>
__device__ __forceinline__ long long launch_lp(const ARGS &AA, long long count)
{
    if constexpr (RAGGED) return (int)blockIdx.x < AA.R.nbin ? (long long)uni(AA.R.order[blockIdx.x]) : -1;
    else return blockIdx.x < count ? (long long)blockIdx.x : -1;
}

// an LP's shape and where its tableau, basis, two-phase working tableau and
// saved costs begin in the packed arrays (wpitch: the widened two-phase pitch;
// a uniform two-phase launch carries it in BArgs::pitch)
struct LpAt {
    int m, n, pitch, wpitch;
    long long toff, boff, woff, coff;
};

template <bool RAGGED, class ARGS>
__device__ __forceinline__ LpAt lp_at(const ARGS &AA, const BArgs &A, long long lp)
{
    if constexpr (RAGGED) {
        const BShape *const sp = AA.R.shape + lp;
        return LpAt{uni(sp->m),    uni(sp->n),    uni(sp->pitch), uni(sp->wpitch),
                    uni(sp->toff), uni(sp->boff), uni(sp->woff),  uni(sp->coff)};
    } else {
        const int E = (A.m + 1) * (A.n + 1);    // fits: every walk counts an LP's elements in an int
        return LpAt{A.m,     A.n,     A.pitch, A.pitch, lp * (long long)E, lp * (long long)A.m,
                    lp * (long long)(A.m + 1) * (A.n + 1 + A.m), lp * (long long)A.n};
    }
}

// RAGGED: launch_lp's and lp_at's.
// MAXINC: bstep's, for lp_batch_run with LP_RULE_MAX_INCREASE.
// DUAL: bstep's, for lp_batch_run with LP_RULE_DUAL; a new call (B_START) ends
// LP_BAD_ARG before any step where the LP is not dual feasible (bdual_start).
template <int WAVES, bool RAGGED = false, bool MAXINC = false, bool DUAL = false>
__global__ __launch_bounds__(64 * WAVES) void k_batch(const std::conditional_t<RAGGED, RArgs, BArgs> AA)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const BArgs &A = AA;
    const long long lp = launch_lp<RAGGED>(AA, A.count);
    if (lp < 0) return;
    BRec *const rp = A.rec + lp;
    const int state = rp->state;
    if (state == B_DONE) return;            // block-uniform: every thread reads the same record

    const int tid = threadIdx.x;
    const LpAt L = lp_at<RAGGED>(AA, A, lp);
    const int m = L.m, n = L.n, pitch = L.pitch;
    const BWalk W = bwalk<NT>(m + 1, n + 1);
    double *const Tl = lds;
    double *const Pl = Tl + (size_t)(m + 1) * pitch;
    double *const Fl = Pl + pitch;
    double *const sc = Fl + (m + 1);
    double *const Tg = A.T + L.toff;
    const lp_tol tol = A.tol;

    // (this loop and the store below are walk()'s, spelled out: through walk() the kernel takes two
    // more SGPRs, 102 in k_batch<4> and in the one-wave max-increase forms, and 7 waves per SIMD, not 8)
    {
        int i = W.i0, j = W.j0;
        for (int e = tid; e < W.E; e += NT) {
            Tl[i * pitch + j] = Tg[e];
            j += W.dj;
            i += W.di;
            if (j >= W.w) { j -= W.w; ++i; }
        }
    }
    __syncthreads();

    BSolve S;
    if (state == B_START) S = solve_start(-Tl[0], A.mode == MODE_SOLVE ? (int)LP_RULE_STANDARD : A.run_rule);
    else S = solve_load(rp);
    const long long npiv_in = S.npiv;
    int status = LP_PIVOTED;
    bool done = false;
    int32_t *const basis = A.basis ? A.basis + L.boff : nullptr;
    long long *const log = A.logcap > 0 ? A.log + lp * A.logcap * 2 : nullptr;

    if constexpr (DUAL) {
        if (state == B_START && bdual_start<WAVES>(Tl, sc, n, tol)) {
            status = LP_BAD_ARG;
            done = true;
        }
    }
    for (long long it = 0; it < A.chunk && !done; ++it)
        done = bstep<WAVES, false, BWalk, false, MAXINC, DUAL>(Tl, Pl, Fl, sc, m, n, pitch, W, tol, A.mode, A.limit,
                                                               S, status, basis, log, A.logcap);

    if (S.npiv != npiv_in) {
        int i = W.i0, j = W.j0;
        for (int e = tid; e < W.E; e += NT) {
            Tg[e] = Tl[i * pitch + j];
            j += W.dj;
            i += W.di;
            if (j >= W.w) { j -= W.w; ++i; }
        }
    }
    if (tid == 0) solve_store(rp, S, status, done);
}

// what a device-placed launch adds: the element updates one launch may apply
// per LP (batch_plan.h: plan_device_chunk)
template <bool RAGGED>
struct DArgs : std::conditional_t<RAGGED, RArgs, BArgs> {
    using Lds = std::conditional_t<RAGGED, RArgs, BArgs>;   // k_batch's args
    long long work;
};

// k_batch for LPs too large for a CU's LDS: one workgroup per
// LP, the tableau read and written in place in device memory, P, F and the
// reduction scratch in LDS.  Records, log, basis and chunk logic are k_batch's;
// there is no load or store phase around the pivots, and a launch stops after
// min(chunk, work / E) pivots, at least one.  No waiting of any kind: every
// loop is bounded by an argument.
//
// Registers: asked to fit 8 waves per SIMD, a CU holds two 16-wave workgroups
// (78 SGPRs, 56 VGPRs, no scratch); without the request the kernel takes 106
// SGPRs, 7 waves per SIMD, and a CU holds one (LPK_BATCH_DEV_OCC8=0: the A/B of
// scripts/place_waves.py).
#ifndef LPK_BATCH_DEV_OCC8
#define LPK_BATCH_DEV_OCC8 1
#endif
#if LPK_BATCH_DEV_OCC8
#define LPK_DEV_BOUNDS(NT) __launch_bounds__(NT, 8)
#else
#define LPK_DEV_BOUNDS(NT) __launch_bounds__(NT)
#endif
template <int WAVES, bool RAGGED = false, bool MAXINC = false, bool DUAL = false>
__global__ LPK_DEV_BOUNDS(64 * WAVES) void k_batch_dev(const DArgs<RAGGED> AA)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const BArgs &A = AA;
    const long long lp = launch_lp<RAGGED>(AA, A.count);
    if (lp < 0) return;
    BRec *const rp = A.rec + lp;
    const int state = uni(rp->state);
    if (state == B_DONE) return;            // block-uniform: every thread reads the same record

    const int tid = threadIdx.x;
    const LpAt L = lp_at<RAGGED>(AA, A, lp);
    const int m = L.m, n = L.n;
    const long long toff = L.toff, boff = L.boff;
    const DWalk W = dwalk<NT>(m + 1, n + 1, (int)(toff & 1));
    double *const Pl = lds;
    double *const Fl = Pl + (n + 1);
    double *const sc = Fl + (m + 1);
    double *const Tg = A.T + toff;
    const lp_tol tol = A.tol;

    BSolve S;
    if (state == B_START) S = solve_start(-Tg[0], A.mode == MODE_SOLVE ? (int)LP_RULE_STANDARD : A.run_rule);
    else S = solve_load(rp);
    __syncthreads();        // every wave has read the record before thread 0 may rewrite it
    int status = LP_PIVOTED;
    bool done = false;
    int32_t *const basis = A.basis ? A.basis + boff : nullptr;
    long long *const log = A.logcap > 0 ? A.log + lp * A.logcap * 2 : nullptr;

    long long chunk = AA.work / W.E;
    chunk = chunk < 1 ? 1 : chunk < A.chunk ? chunk : A.chunk;
    if constexpr (DUAL) {
        if (state == B_START && bdual_start<WAVES>(Tg, sc, n, tol)) {
            status = LP_BAD_ARG;
            done = true;
        }
    }
    for (long long it = 0; it < chunk && !done; ++it)
        done = bstep<WAVES, true, DWalk, false, MAXINC, DUAL>(Tg, Pl, Fl, sc, m, n, n + 1, W, tol, A.mode, A.limit, S,
                                                              status, basis, log, A.logcap);

    if (tid == 0) solve_store(rp, S, status, done);
}

// what a teamed launch adds: the LPs' second buffer, laid out
// as BArgs::T; the record arrays of this launch (BArgs::rec is unused); and the
// workgroup table (batch_plan.h: plan_team_table), one entry per block
template <bool RAGGED>
struct MArgs : std::conditional_t<RAGGED, RArgs, BArgs> {
    double *T2;
    const BRec *rec_in;
    BRec *rec_out;
    const TeamWG *wg;
    int nwg;
};

// k_batch_dev for an LP that a team of workgroups shares: one
// launch applies at most ONE pivot to every unfinished teamed LP.  Block b is
// rank wg[b].rank of the team of LP wg[b].lp.  Every workgroup of a team reads
// the same record and the same current buffer and runs the same bstep, so all
// reach the same C, R, status and counters; each writes only its own range of
// the other buffer, and rank 0 alone writes the log, the basis and the output
// record.  BRec::buf says which buffer is current; it flips only when a pivot
// was applied.  Rank 0 writes the LP's output record in every launch, finished
// or not, so both record arrays read B_DONE from the second launch after the
// last pivot on.  See bpivot_dev (TWalk) for why nothing here waits or synchronises
// beyond the workgroup.
#ifndef LPK_TEAM_OCC8
#define LPK_TEAM_OCC8 1
#endif
#if LPK_TEAM_OCC8
#define LPK_TEAM_BOUNDS(NT) __launch_bounds__(NT, 8)
#else
#define LPK_TEAM_BOUNDS(NT) __launch_bounds__(NT)
#endif
template <int WAVES, bool RAGGED = false>
__global__ LPK_TEAM_BOUNDS(64 * WAVES) void k_batch_team(const MArgs<RAGGED> AA)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const BArgs &A = AA;
    if ((int)blockIdx.x >= AA.nwg) return;
    const TeamWG *const wp = AA.wg + blockIdx.x;
    const long long lp = uni(wp->lp);
    const int rank = uni(wp->rank), e0 = uni(wp->e0), e1 = uni(wp->e1);
    const BRec *const rp = AA.rec_in + lp;
    BRec *const op = AA.rec_out + lp;
    const int tid = threadIdx.x;
    const int state = uni(rp->state);
    if (state == B_DONE) {                  // block-uniform: every thread reads the same record
        if (rank == 0 && tid == 0) *op = *rp;
        return;
    }

    const LpAt L = lp_at<RAGGED>(AA, A, lp);
    const int m = L.m, n = L.n;
    const long long toff = L.toff, boff = L.boff;
    const int buf = state == B_START ? 0 : uni(rp->buf);
    const double *const Tin = (buf ? AA.T2 : A.T) + toff;
    const TWalk W = twalk<NT>(n + 1, e0, e1, (int)((toff + e0) & 1), (buf ? A.T : AA.T2) + toff);
    double *const Pl = lds;
    double *const Fl = Pl + (n + 1);
    double *const sc = Fl + (m + 1);
    const lp_tol tol = A.tol;

    BSolve S;
    if (state == B_START) S = solve_start(-Tin[0], A.mode == MODE_SOLVE ? (int)LP_RULE_STANDARD : A.run_rule);
    else S = solve_load(rp);
    int status = LP_PIVOTED;
    // the log and the basis are rank 0's
    int32_t *const basis = A.basis && rank == 0 ? A.basis + boff : nullptr;
    long long *const log = A.logcap > 0 ? A.log + lp * A.logcap * 2 : nullptr;
    const bool done = bstep<WAVES, true, TWalk, true>(const_cast<double *>(Tin), Pl, Fl, sc, m, n, n + 1, W, tol,
                                                      A.mode, A.limit, S, status, basis, log,
                                                      rank == 0 ? A.logcap : 0);
    if (rank == 0 && tid == 0) solve_store<true>(op, S, status, done, W.applied ? buf ^ 1 : buf);
}

// After the last launch of a call: a teamed LP whose current buffer is the
// second one goes back to BArgs::T, each workgroup of the table copying its
// own range, so that every other call finds the LP where it always is.
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_team_home(const MArgs<RAGGED> AA)
{
    const BArgs &A = AA;
    if ((int)blockIdx.x >= AA.nwg) return;
    const TeamWG *const wp = AA.wg + blockIdx.x;
    const long long lp = uni(wp->lp);
    if (uni(AA.rec_in[lp].buf) == 0) return;
    const long long toff = lp_at<RAGGED>(AA, A, lp).toff;
    const int e1 = uni(wp->e1);
    for (int e = uni(wp->e0) + (int)threadIdx.x; e < e1; e += 256) A.T[toff + e] = AA.T2[toff + e];
}

// ---------------------------------------------------------------------------
// Two-phase solve (lp_twophase_solve): Simplex._find_bfs
// (simplex.py:36-108) as oracle/phase1.py restates it, then Simplex.solve, per
// LP and without the tableau leaving the device.  The LDS rows are pitched for
// the widest artificial problem (n + 1 + m columns); each LP walks its own
// live width n + 1 + k and its live rows.  Between launches the working
// tableau lives in W (rows at ww = n + 1 + m doubles), the basis in A.B.basis,
// the saved costs in origc and the stage in TRec; A.B.T is written only when
// an LP finishes phase 2.
// ---------------------------------------------------------------------------
constexpr int T_DROPPED = -2;   // basis mark of a linearly dependent row (drive-out)

struct TRec {
    int32_t stage;    // LP_STAGE_*
    int32_t k;        // artificial columns
    int32_t rows;     // live rows (m, then m' after the compaction)
    int32_t cursor;   // drive-out: next row to look at
    long long ninit;  // phase-1 pivots so far
    double orig_z;
};

struct TArgs {
    BArgs B;          // basis non-null; pitch is the widened one; mode unused
    double *W;        // count x (m+1) x ww
    double *origc;    // count x n
    TRec *trec;       // count
    int ww;           // n + 1 + m of a uniform batch; set by the host, read by no kernel
};

struct RTArgs : TArgs {
    RBin R;
};

// copy the live rows x w tableau between LDS (row pitch) and global (row ld)
template <int NT, bool TO_LDS>
__device__ __forceinline__ void tcopy(double *Tl, int pitch, double *G, int ld, const BWalk &W)
{
    walk<NT>(W, [&](int, int i, int j) {
        if constexpr (TO_LDS) Tl[i * pitch + j] = G[(long long)i * ld + j];
        else G[(long long)i * ld + j] = Tl[i * pitch + j];
    });
}

// ---- k_twophase's shared stages.  k_twophase and k_twophase_dev are one state
// machine over two storages: the LP's rows in LDS at the launch's pitch
// (LdsRows), or its slot of W at the live width.  Stages 1, 3, 7 and 8 -- the
// flip and scan, building the artificial problem, the compaction and restoring
// row 0 -- differ in substance; the rest is here.  Only k_twophase calls these:
// k_twophase_dev written over them measured 3 % slower at its smaller shapes
// (profiles/r17/README.md), so it keeps the same stages spelled out; a change
// to one of them is made there too.  Every function below is called by the
// whole workgroup, from block-uniform control flow.

// TRec in registers
struct TStage {
    int stage, k, m, cursor;
    long long ninit;
    double orig_z;
};

__device__ __forceinline__ TStage stage_load(const TRec *tp)
{
    return TStage{uni(tp->stage), uni(tp->k), uni(tp->rows), uni(tp->cursor), tp->ninit, tp->orig_z};
}

__device__ __forceinline__ void stage_store(TRec *tp, const TStage &Q)
{
    tp->stage = Q.stage;
    tp->k = Q.k;
    tp->rows = Q.m;
    tp->cursor = Q.cursor;
    tp->ninit = Q.ninit;
    tp->orig_z = Q.orig_z;
}

// the drive-out's rows and pivot: T[i * ld + j] is element (i, j)
template <int NT>
struct LdsRows {
    double *T, *Pl, *Fl;
    int m0, ld;
    const BWalk &W;
    __device__ __forceinline__ void pivot(int nl, long long R, long long C, double a) const
    {
        bpivot<NT>(T, Pl, Fl, m0, nl, ld, W, R, C, a);
    }
};

// rows without a basic column get the artificial columns n, n + 1, ... in row
// order; returns their count k.  Follows the barrier that makes the scan's
// Bl whole.
__device__ __forceinline__ int tp_artificials(int32_t *Bl, double *sc, int m0, int n)
{
    if (threadIdx.x == 0) {
        int cnt = 0;
#pragma unroll 1
        for (int i = 0; i < m0; ++i)
            if (Bl[i] == INT_MAX) Bl[i] = n + cnt++;
        reinterpret_cast<int *>(sc)[0] = cnt;
    }
    __syncthreads();
    return uni(reinterpret_cast<int *>(sc)[0]);
}

// 6. one step of the drive-out's cursor (Q.cursor < m0): a basic artificial
// leaves on the first structural column with |a| > tol.pivot, or its row is
// linearly dependent
enum { DRIVE_NEXT, DRIVE_PIVOTED, DRIVE_FAILED };
template <int WAVES, class ROWS>
__device__ __forceinline__ int tp_drive(const ROWS &X, int32_t *Bl, double *sc, TStage &Q, int n,
                                        const lp_tol &tol, long long *log, long long logcap)
{
    constexpr int NT = 64 * WAVES;
    const int tid = threadIdx.x;
    const int c = uni(Bl[Q.cursor]);
    if (c < n) {
        ++Q.cursor;
        return DRIVE_NEXT;
    }
    const int R = Q.cursor + 1;
    if (fabs(X.T[R * X.ld]) > tol.zero) return DRIVE_FAILED;      // "invalid artificial solution"
    long long f = NONE;
#pragma unroll 1
    for (int j = 1 + tid; j <= n; j += NT)
        if (fabs(X.T[R * X.ld + j]) > tol.pivot && f == NONE) f = j;
    const long long C = bmin_ll<WAVES>(f, sc);
    if (C == NONE) {
        if (tid == 0) Bl[Q.cursor] = T_DROPPED;
        ++Q.cursor;
        return DRIVE_NEXT;
    }
    const double a = X.T[R * X.ld + C];
    if (a != 0.0) X.pivot(n + Q.k, R, C, a);
    if (tid == 0) {
        Bl[Q.cursor] = (int32_t)(C - 1);
        if (Q.ninit < logcap) {
            log[Q.ninit * 2] = Q.cursor;
            log[Q.ninit * 2 + 1] = C - 1;
        }
    }
    ++Q.ninit;
    ++Q.cursor;
    return DRIVE_PIVOTED;
}

// 7. (the basis' part) the dropped rows' marks squeezed out, -1 behind the kept ones
__device__ __forceinline__ void tp_compact_basis(int32_t *Bl, int m0)
{
    if (threadIdx.x == 0) {
        int e = 0;
#pragma unroll 1
        for (int i = 0; i < m0; ++i)
            if (Bl[i] != T_DROPPED) Bl[e++] = Bl[i];
#pragma unroll 1
        for (; e < m0; ++e) Bl[e] = -1;
    }
}

// 4./5. the artificial solve ended with `status`, T = the tableau (T[0] its
// objective entry).  True: the call ends here; else the drive-out begins.
__device__ __forceinline__ bool tp_artificial_ended(TStage &Q, const BSolve &S, int &status, const double *T,
                                                    const lp_tol &tol)
{
    Q.ninit = S.npiv;
    if (status != LP_OPTIMAL) return true;      // cap, or the oracle's "unbounded artificial problem"
    if (fabs(T[0]) > tol.zero) {
        status = LP_INFEASIBLE;
        return true;
    }
    status = LP_PIVOTED;
    Q.stage = LP_STAGE_DRIVE_OUT;
    Q.cursor = 0;
    __syncthreads();                            // the last pivot's basis entry
    return false;
}

// the basis and both records at the end of a launch (an unfinished drive-out
// keeps its marks for the next launch)
template <int NT>
__device__ __forceinline__ void tp_finish(BRec *rp, TRec *tp, int32_t *Bg, const int32_t *Bl, int m0,
                                          const BSolve &S, const TStage &Q, int status, bool done)
{
#pragma unroll 1
    for (int i = threadIdx.x; i < m0; i += NT) Bg[i] = done && Bl[i] == T_DROPPED ? -1 : Bl[i];
    if (threadIdx.x == 0) {
        solve_store(rp, S, status, done);
        stage_store(tp, Q);
    }
}

// RAGGED as in k_batch; the LP's rows sit at its own widened pitch and its
// working tableau, saved costs and basis at the table's woff, coff and boff.
template <int WAVES, bool RAGGED = false>
__global__ __launch_bounds__(64 * WAVES) void k_twophase(const std::conditional_t<RAGGED, RTArgs, TArgs> TT)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const TArgs &TA = TT;
    const BArgs &A = TA.B;
    const long long lp = launch_lp<RAGGED>(TT, A.count);
    if (lp < 0) return;
    BRec *const rp = A.rec + lp;
    const int state = uni(rp->state);
    if (state == B_DONE) return;            // block-uniform

    const int tid = threadIdx.x;
    const LpAt L = lp_at<RAGGED>(TT, A, lp);
    const int m0 = L.m, n = L.n, pitch = L.wpitch, ww = n + 1 + m0;
    double *const Tl = lds;
    double *const Pl = Tl + (size_t)(m0 + 1) * pitch;
    double *const Fl = Pl + pitch;
    double *const sc = Fl + (m0 + 1);
    int32_t *const Bl = reinterpret_cast<int32_t *>(sc + 16);     // m0 basic columns
    double *const Tg = A.T + L.toff;
    double *const Wg = TA.W + L.woff;
    double *const Cg = TA.origc + L.coff;
    int32_t *const Bg = A.basis + L.boff;
    TRec *const tp = TA.trec + lp;
    const lp_tol tol = A.tol;

    TStage Q;
    BSolve S;
    BWalk W;
    if (state == B_START) {
        Q = TStage{LP_STAGE_PHASE2, 0, m0, 0, 0, 0.0};
        W = bwalk<NT>(m0 + 1, n + 1);
        tcopy<NT, true>(Tl, pitch, Tg, n + 1, W);
        __syncthreads();
        // 1. rows with b_i < 0 times -1, the whole row (signed zeros kept)
#pragma unroll 1
        for (int i = tid; i < m0; i += NT) {
            Fl[1 + i] = Tl[(1 + i) * pitch] < 0.0 ? 1.0 : 0.0;
            Bl[i] = INT_MAX;
        }
        if (tid == 0) Fl[0] = 0.0;
        __syncthreads();
        walk<NT, true>(W, [&](int, int i, int j) {
            if (Fl[i] != 0.0) Tl[i * pitch + j] = -Tl[i * pitch + j];
        });
        __syncthreads();
        // 2. Tableau.isCanonical's basic columns, lanes over columns; the
        // lowest column wins a row
#pragma unroll 1
        for (int j = tid; j < n; j += NT) {
            if (!(Tl[1 + j] == 0.0)) continue;
            int onei = -1;
#pragma unroll 1
            for (int i = 0; i < m0; ++i)
                if (Tl[(1 + i) * pitch + 1 + j] == 1.0) {
                    onei = i;
                    break;
                }
            if (onei < 0) continue;
            bool unit = true;
#pragma unroll 1
            for (int i = 0; i < m0; ++i)
                if (i != onei && !(Tl[(1 + i) * pitch + 1 + j] == 0.0)) unit = false;
            if (unit) atomicMin(&Bl[onei], j);
        }
        __syncthreads();
        // rows without one get the artificial columns n, n + 1, ... in row order
        Q.k = tp_artificials(Bl, sc, m0, n);
        if (Q.k == 0) {
            Q.stage = LP_STAGE_PHASE2;
        } else {
            // 3. the artificial problem on the m0 x (n + k) working shape
            Q.stage = LP_STAGE_ARTIFICIAL;
            Q.orig_z = -Tl[0] + 0.0;
#pragma unroll 1
            for (int j = 1 + tid; j <= n; j += NT) Cg[j - 1] = Tl[j];
#pragma unroll 1
            for (int e = tid; e < m0 * Q.k; e += NT) Tl[(1 + e / Q.k) * pitch + n + 1 + e % Q.k] = 0.0;
            __syncthreads();
#pragma unroll 1
            for (int j = tid; j <= n + Q.k; j += NT) Tl[j] = j == 0 ? -0.0 : 0.0;
            __syncthreads();
#pragma unroll 1
            for (int i = tid; i < m0; i += NT) {
                const int c = Bl[i];
                if (c >= n) {
                    Tl[(1 + i) * pitch + 1 + c] = 1.0;
                    Tl[1 + c] = 1.0;
                }
            }
            __syncthreads();
#pragma unroll 1
            for (int j = tid; j <= n + Q.k; j += NT) {       // a lane owns its columns: rows in order
                double x = Tl[j];
#pragma unroll 1
                for (int i = 0; i < m0; ++i)
                    if (Bl[i] >= n) x = x + (-1.0 * Tl[(1 + i) * pitch + j]);
                Tl[j] = x;
            }
            W = bwalk<NT>(m0 + 1, n + 1 + Q.k);
            __syncthreads();
        }
        S = solve_start(-Tl[0], LP_RULE_STANDARD);
    } else {
        Q = stage_load(tp);
        S = solve_load(rp);
        W = bwalk<NT>(Q.m + 1, Q.stage == LP_STAGE_PHASE2 ? n + 1 : n + 1 + Q.k);
        tcopy<NT, true>(Tl, pitch, Wg, ww, W);
#pragma unroll 1
        for (int i = tid; i < m0; i += NT) Bl[i] = Bg[i];
        __syncthreads();
    }

    int status = LP_PIVOTED;
    bool done = false;
    long long *const log = A.logcap > 0 ? A.log + lp * A.logcap * 2 : nullptr;

    // One pivot at the most per iteration, in whichever stage the LP is; the
    // stage, the cursor and every test below are block-uniform.
    for (long long it = 0; it < A.chunk;) {
        if (Q.stage == LP_STAGE_DRIVE_OUT) {
            if (Q.cursor < m0) {
                // 6. the cursor's next row
                const int r = tp_drive<WAVES>(LdsRows<NT>{Tl, Pl, Fl, m0, pitch, W}, Bl, sc, Q, n, tol, log, A.logcap);
                if (r == DRIVE_FAILED) {
                    status = LP_PHASE1_FAILED;
                    done = true;
                    break;
                }
                if (r == DRIVE_PIVOTED) ++it;
                continue;
            }
            // 7. drop the dependent rows (a lane owns its columns and rows move
            // up in order, so a row is read before it is overwritten) and the
            // artificial columns; snap every kept |b_i| <= tol.zero to +0
            __syncthreads();
            int d = 0;
#pragma unroll 1
            for (int i = 0; i < m0; ++i) {
                if (uni(Bl[i]) == T_DROPPED) continue;
                if (d != i)
#pragma unroll 1
                    for (int j = tid; j <= n; j += NT) Tl[(1 + d) * pitch + j] = Tl[(1 + i) * pitch + j];
                ++d;
            }
            Q.m = d;
            __syncthreads();
            tp_compact_basis(Bl, m0);
#pragma unroll 1
            for (int i = tid; i < Q.m; i += NT)
                if (fabs(Tl[(1 + i) * pitch]) <= tol.zero) Tl[(1 + i) * pitch] = 0.0;
            // 8. the objective back, then each basic column's cost eliminated:
            // numpy's T[0] += s * T[1+i], the product rounded before the add
            if (tid == 0) Tl[0] = -Q.orig_z;
#pragma unroll 1
            for (int j = 1 + tid; j <= n; j += NT) Tl[j] = Cg[j - 1];
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < Q.m; ++i) {
                const double s = -Tl[1 + uni(Bl[i])];
                __syncthreads();
#pragma unroll 1
                for (int j = tid; j <= n; j += NT)
                    Tl[j] = __dadd_rn(Tl[j], __dmul_rn(s, Tl[(1 + i) * pitch + j]));
                __syncthreads();
            }
            // 9. phase 2 on the m' x n tableau
            Q.stage = LP_STAGE_PHASE2;
            W = bwalk<NT>(Q.m + 1, n + 1);
            S = solve_start(-Tl[0], LP_RULE_STANDARD);
            continue;
        }
        const bool p2 = Q.stage == LP_STAGE_PHASE2;
        const long long base = p2 ? Q.ninit : 0;
        const bool fin = bstep<WAVES>(Tl, Pl, Fl, sc, Q.m, p2 ? n : n + Q.k, pitch, W, tol, MODE_SOLVE,
                                      A.limit, S, status, Bl, log + base * 2, A.logcap - base);
        ++it;
        if (!fin) continue;
        if (p2) {
            done = true;
            break;
        }
        // 4./5. the artificial solve ended
        if (tp_artificial_ended(Q, S, status, Tl, tol)) {
            done = true;
            break;
        }
    }

    __syncthreads();
    if (Q.stage == LP_STAGE_ARTIFICIAL) Q.ninit = S.npiv;
    if (done && Q.stage == LP_STAGE_PHASE2) {
        // the final (m'+1) x (n+1) tableau, the dropped rows' places +0.0
        tcopy<NT, false>(Tl, pitch, Tg, n + 1, W);
#pragma unroll 1
        for (int e = (Q.m + 1) * (n + 1) + tid; e < (m0 + 1) * (n + 1); e += NT) Tg[e] = 0.0;
    } else if (!done) {
        tcopy<NT, false>(Tl, pitch, Wg, ww, W);
    }
    tp_finish<NT>(rp, tp, Bg, Bl, m0, S, Q, status, done);
}

// ---------------------------------------------------------------------------
// Two-phase solve of device-placed LPs (lp_phased_solve):
// k_twophase's stages on an LP whose widened tableau does not fit a CU's LDS.
// The working tableau lives in the LP's slot of W for the whole call,
// contiguous at its LIVE width -- n + 1 + k during the artificial solve and
// the drive-out, n + 1 in phase 2 -- because bstep<DEV> / bpivot_dev walk the
// LP flat, pitch = width.  A launch has no load and no store phase.  P (at the
// widest width n + 1 + m), F, the reduction scratch and the basis are in LDS.
//
// Visibility (the argument of 4j): within a launch this LP's bytes of W, T,
// origc and basis are read and written by this workgroup only, on one CU, so
// __syncthreads()'s workgroup-scope release / acquire orders every store below
// before the loads that follow its barrier; the kernel boundary orders the
// launches.  No agent-scope fence, no cache-bypassing access, no global
// atomic, no flag and no waiting: every loop is bounded by an argument.
// ---------------------------------------------------------------------------

// what a phased launch adds: the element updates one launch may apply per LP,
// taken on the widened element count (batch_plan.h: plan_phased_chunk)
template <bool RAGGED>
struct PArgs : std::conditional_t<RAGGED, RTArgs, TArgs> {
    using Lds = std::conditional_t<RAGGED, RTArgs, TArgs>;  // k_twophase's args
    long long work;
};

// Registers: the occupancy request of k_batch_dev is an A/B
// build here (LPK_PHASED_OCC8=1, scripts/phased_waves.py)
#ifndef LPK_PHASED_OCC8
#define LPK_PHASED_OCC8 0
#endif
#if LPK_PHASED_OCC8
#define LPK_PHASED_BOUNDS(NT) __launch_bounds__(NT, 8)
#else
#define LPK_PHASED_BOUNDS(NT) __launch_bounds__(NT)
#endif
template <int WAVES, bool RAGGED = false>
__global__ LPK_PHASED_BOUNDS(64 * WAVES) void k_twophase_dev(const PArgs<RAGGED> TT)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const TArgs &TA = TT;
    const BArgs &A = TA.B;
    long long lp;
    if constexpr (RAGGED) {
        if ((int)blockIdx.x >= TT.R.nbin) return;
        lp = uni(TT.R.order[blockIdx.x]);
    } else {
        lp = blockIdx.x;
        if (lp >= A.count) return;
    }
    BRec *const rp = A.rec + lp;
    const int state = uni(rp->state);
    if (state == B_DONE) return;            // block-uniform

    const int tid = threadIdx.x;
    int m0, n;
    long long toff, woff, coff, boff;
    if constexpr (RAGGED) {
        const BShape *const sp = TT.R.shape + lp;
        m0 = uni(sp->m);
        n = uni(sp->n);
        toff = uni(sp->toff);
        woff = uni(sp->woff);
        coff = uni(sp->coff);
        boff = uni(sp->boff);
    } else {
        m0 = A.m;
        n = A.n;
        toff = lp * (long long)(m0 + 1) * (n + 1);
        woff = lp * (long long)(m0 + 1) * (n + 1 + m0);
        coff = lp * (long long)n;
        boff = lp * (long long)m0;
    }
    double *const Pl = lds;                                      // n + 1 + m0
    double *const Fl = Pl + (n + 1 + m0);                        // m0 + 1
    double *const sc = Fl + (m0 + 1);
    int32_t *const Bl = reinterpret_cast<int32_t *>(sc + 16);    // m0 basic columns
    double *const Tg = A.T + toff;
    double *const Wg = TA.W + woff;
    double *const Cg = TA.origc + coff;
    int32_t *const Bg = A.basis + boff;
    TRec *const tp = TA.trec + lp;
    const lp_tol tol = A.tol;
    const int head = (int)(woff & 1);       // the slot may start at an odd double
    const int w0 = n + 1;

    int stage, k, m, cursor;
    long long ninit;
    double orig_z;
    BSolve S;
    if (state == B_START) {
        m = m0;
        cursor = 0;
        ninit = 0;
        orig_z = 0.0;
        // 1. the sign of every row with b_i < 0, kept as a flag: the uploaded
        // tableau is scanned with the flags applied on the fly, and W is
        // written once, at the pitch the scan decides
#pragma unroll 1
        for (int i = tid; i < m0; i += NT) {
            Fl[1 + i] = Tg[(1 + i) * w0] < 0.0 ? 1.0 : 0.0;
            Bl[i] = INT_MAX;
        }
        if (tid == 0) Fl[0] = 0.0;
        __syncthreads();
        // 2. Tableau.isCanonical's basic columns, lanes over columns (a row of
        // the tableau is read coalesced); the lowest column wins a row
#pragma unroll 1
        for (int j = tid; j < n; j += NT) {
            if (!(Tg[1 + j] == 0.0)) continue;
            int onei = -1;
#pragma unroll 1
            for (int i = 0; i < m0; ++i) {
                const double x = Tg[(1 + i) * w0 + 1 + j];
                if ((Fl[1 + i] != 0.0 ? -x : x) == 1.0) {
                    onei = i;
                    break;
                }
            }
            if (onei < 0) continue;
            bool unit = true;
#pragma unroll 1
            for (int i = 0; i < m0; ++i)
                if (i != onei && !(Tg[(1 + i) * w0 + 1 + j] == 0.0)) unit = false;     // -x == 0 as x == 0
            if (unit) atomicMin(&Bl[onei], j);
        }
        __syncthreads();
        // rows without one get the artificial columns n, n + 1, ... in row order
        if (tid == 0) {
            int cnt = 0;
#pragma unroll 1
            for (int i = 0; i < m0; ++i)
                if (Bl[i] == INT_MAX) Bl[i] = n + cnt++;
            reinterpret_cast<int *>(sc)[0] = cnt;
        }
        __syncthreads();
        k = uni(reinterpret_cast<int *>(sc)[0]);
        stage = k == 0 ? LP_STAGE_PHASE2 : LP_STAGE_ARTIFICIAL;
        if (k > 0) {
            orig_z = -Tg[0] + 0.0;
#pragma unroll 1
            for (int j = 1 + tid; j <= n; j += NT) Cg[j - 1] = Tg[j];
        }
        // 3. W at pitch n + 1 + k: the flipped rows (signed zeros kept), the
        // artificial columns, and for k > 0 the artificial costs in row 0
        {
            const BWalk X = bwalk<NT>(m0 + 1, n + 1 + k);
            int i = X.i0, j = X.j0;
#pragma unroll 1
            for (int e = tid; e < X.E; e += NT) {
                double x;
                if (j > n) x = i == 0 || Bl[i - 1] == j - 1 ? 1.0 : 0.0;
                else if (i == 0 && k > 0) x = j == 0 ? -0.0 : 0.0;
                else {
                    x = Tg[i * w0 + j];
                    if (Fl[i] != 0.0) x = -x;
                }
                Wg[e] = x;
                j += X.dj;
                i += X.di;
                if (j >= X.w) { j -= X.w; ++i; }
            }
        }
        __syncthreads();        // W is whole before a lane reads the rows of its columns
        if (k > 0) {
            const int w = n + 1 + k;
#pragma unroll 1
            for (int j = tid; j < w; j += NT) {            // a lane owns its columns: rows in order
                double x = Wg[j];
#pragma unroll 1
                for (int i = 0; i < m0; ++i)
                    if (Bl[i] >= n) x = x + (-1.0 * Wg[(1 + i) * w + j]);
                Wg[j] = x;
            }
            __syncthreads();    // row 0 is whole before the first selection reads it
        }
        S.npiv = S.nstd = S.stuck = 0;
        S.z0 = -Wg[0];
        S.rule = LP_RULE_STANDARD;
    } else {
        stage = uni(tp->stage);
        k = uni(tp->k);
        m = uni(tp->rows);
        cursor = uni(tp->cursor);
        ninit = tp->ninit;
        orig_z = tp->orig_z;
        S.npiv = rp->npiv;
        S.nstd = rp->nstd;
        S.stuck = rp->stuck;
        S.z0 = rp->z0;
        S.rule = rp->rule;
#pragma unroll 1
        for (int i = tid; i < m0; i += NT) Bl[i] = Bg[i];
    }
    __syncthreads();        // every wave has read the records before thread 0 may rewrite them; Bl is whole
    DWalk DW = dwalk<NT>(m + 1, stage == LP_STAGE_PHASE2 ? n + 1 : n + 1 + k, head);

    int status = LP_PIVOTED;
    bool done = false;
    long long *const log = A.logcap > 0 ? A.log + lp * A.logcap * 2 : nullptr;
    long long chunk = TT.work / ((long long)(m0 + 1) * (n + 1 + m0));
    chunk = chunk < 1 ? 1 : chunk < A.chunk ? chunk : A.chunk;

    // One pivot at the most per iteration, in whichever stage the LP is; the
    // stage, the cursor and every test below are block-uniform: each value
    // comes from a record, from LDS or from an address of W that every
    // thread reads alike after the barrier that followed its last store.
    for (long long it = 0; it < chunk;) {
        if (stage == LP_STAGE_DRIVE_OUT) {
            const int w = n + 1 + k;
            if (cursor < m0) {
                // 6. a basic artificial leaves on the first structural column
                // with |a| > tol.pivot, or its row is linearly dependent
                const int c = uni(Bl[cursor]);
                if (c < n) {
                    ++cursor;
                    continue;
                }
                const int R = cursor + 1;
                if (fabs(Wg[R * w]) > tol.zero) {          // "invalid artificial solution"
                    status = LP_PHASE1_FAILED;
                    done = true;
                    break;
                }
                long long f = NONE;
#pragma unroll 1
                for (int j = 1 + tid; j <= n; j += NT)
                    if (fabs(Wg[R * w + j]) > tol.pivot && f == NONE) f = j;
                const long long C = bmin_ll<WAVES>(f, sc);
                if (C == NONE) {
                    if (tid == 0) Bl[cursor] = T_DROPPED;
                    ++cursor;
                    continue;
                }
                const double a = Wg[R * w + C];
                if (a != 0.0) {
                    // no ratio test ran, so column C is staged here; the
                    // barrier puts F[1..m0] before bpivot_dev's update pass
#pragma unroll 1
                    for (int i = 1 + tid; i <= m0; i += NT) Fl[i] = Wg[i * w + C];
                    __syncthreads();
                    bpivot_dev<NT>(Wg, Pl, Fl, n + k, DW, R, C, a);
                }
                if (tid == 0) {
                    Bl[cursor] = (int32_t)(C - 1);
                    if (ninit < A.logcap) {
                        log[ninit * 2] = cursor;
                        log[ninit * 2 + 1] = C - 1;
                    }
                }
                ++ninit;
                ++cursor;
                ++it;
                continue;
            }
            // 7. drop the dependent rows and the artificial columns: kept row
            // i moves to row d <= i and the pitch narrows from w to n + 1, so
            // every element moves to a lower address.  Row d's new place ends
            // below (2 + d)(n + 1) <= (2 + i) w, where the next unread row
            // begins, but it can overlap row i's own old place, which another
            // lane may not have read yet: each row goes through P, a barrier
            // between its reads and its writes, and one before P is reused.
            // Every kept |b_i| <= tol.zero is snapped to +0 on the way.
            __syncthreads();
            int d = 0;
#pragma unroll 1
            for (int i = 0; i < m0; ++i) {
                if (uni(Bl[i]) == T_DROPPED) continue;
#pragma unroll 1
                for (int j = tid; j <= n; j += NT) {
                    const double x = Wg[(1 + i) * w + j];
                    Pl[j] = j == 0 && fabs(x) <= tol.zero ? 0.0 : x;
                }
                __syncthreads();
#pragma unroll 1
                for (int j = tid; j <= n; j += NT) Wg[(1 + d) * w0 + j] = Pl[j];
                __syncthreads();
                ++d;
            }
            m = d;
            __syncthreads();    // a trailing dropped row ends without a barrier: every wave has read the marks
            if (tid == 0) {
                int e = 0;
#pragma unroll 1
                for (int i = 0; i < m0; ++i)
                    if (Bl[i] != T_DROPPED) Bl[e++] = Bl[i];
#pragma unroll 1
                for (; e < m0; ++e) Bl[e] = -1;
            }
            // 8. the objective back, then each basic column's cost eliminated:
            // numpy's T[0] += s * T[1+i], the product rounded before the add.
            // Row 0 is built in P and stored once.
            if (tid == 0) Pl[0] = -orig_z;
#pragma unroll 1
            for (int j = 1 + tid; j <= n; j += NT) Pl[j] = Cg[j - 1];
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < m; ++i) {
                const double s = -Pl[1 + uni(Bl[i])];
                __syncthreads();
#pragma unroll 1
                for (int j = tid; j <= n; j += NT)
                    Pl[j] = __dadd_rn(Pl[j], __dmul_rn(s, Wg[(1 + i) * w0 + j]));
                __syncthreads();
            }
#pragma unroll 1
            for (int j = tid; j <= n; j += NT) Wg[j] = Pl[j];
            __syncthreads();    // row 0 is in W before P is reused and the selection reads it
            // 9. phase 2 on the m' x n tableau
            stage = LP_STAGE_PHASE2;
            DW = dwalk<NT>(m + 1, n + 1, head);
            S.npiv = S.nstd = S.stuck = 0;
            S.z0 = -Wg[0];
            S.rule = LP_RULE_STANDARD;
            continue;
        }
        const bool p2 = stage == LP_STAGE_PHASE2;
        const long long base = p2 ? ninit : 0;
        const int nl = p2 ? n : n + k;
        const bool fin = bstep<WAVES, true, DWalk>(Wg, Pl, Fl, sc, m, nl, nl + 1, DW, tol, MODE_SOLVE, A.limit, S,
                                                   status, Bl, log + base * 2, A.logcap - base);
        ++it;
        if (!fin) continue;
        if (p2) {
            done = true;
            break;
        }
        // 4./5. the artificial solve ended
        ninit = S.npiv;
        if (status != LP_OPTIMAL) {             // cap, or the oracle's "unbounded artificial problem"
            done = true;
            break;
        }
        if (fabs(Wg[0]) > tol.zero) {
            status = LP_INFEASIBLE;
            done = true;
            break;
        }
        status = LP_PIVOTED;
        stage = LP_STAGE_DRIVE_OUT;
        cursor = 0;
        __syncthreads();                        // the last pivot's basis entry
    }

    __syncthreads();            // the last pivot's stores to W and to Bl
    if (stage == LP_STAGE_ARTIFICIAL) ninit = S.npiv;
    if (done && stage == LP_STAGE_PHASE2) {
        // the final (m'+1) x (n+1) tableau, the dropped rows' places +0.0; an
        // LP that ends before phase 2 keeps the uploaded bits
        const int E = (m + 1) * w0;
#pragma unroll 1
        for (int e = tid; e < E; e += NT) Tg[e] = Wg[e];
#pragma unroll 1
        for (int e = E + tid; e < (m0 + 1) * w0; e += NT) Tg[e] = 0.0;
    }
    // (an unfinished drive-out keeps its marks for the next launch)
#pragma unroll 1
    for (int i = tid; i < m0; i += NT) Bg[i] = done && Bl[i] == T_DROPPED ? -1 : Bl[i];
    if (tid == 0) {
        rp->status = status;
        rp->state = done ? B_DONE : B_RUNNING;
        rp->rule = S.rule;
        rp->npiv = S.npiv;
        rp->nstd = S.nstd;
        rp->stuck = S.stuck;
        rp->z0 = S.z0;
        tp->stage = stage;
        tp->k = k;
        tp->rows = m;
        tp->cursor = cursor;
        tp->ninit = ninit;
        tp->orig_z = orig_z;
    }
}

// T[0][0] of every LP of a ragged batch (lp_batch_objective)
__global__ void k_gather_z(const double *T, const BShape *shape, double *z, long long count)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) z[i] = T[shape[i].toff];
}

// ---------------------------------------------------------------------------
// Batch solutions on the device (lp_solution_canonical / lp_solution_gather;
// DESIGN.md 4m).  Flat kernels over the packed stack as stored: a lane is one
// tableau column (column 0 included) or one basis entry of one LP of the
// window [first, first + count).  No workgroup reads what another wrote in
// the same launch: the canonical scan is three launches on the batch's stream.
// ---------------------------------------------------------------------------
struct SArgs {
    const double *T;            // the packed tableaux (BArgs::T)
    int32_t *basis;             // the packed basis (BArgs::basis)
    const BShape *shape;        // ragged: one per LP of the batch; else null
    long long first, count;     // the window
    long long lanes;            // of this launch
    long long nbasis;           // basis entries of the window
    int m, n;                   // uniform batch only
    int32_t *flags;             // canonical: count, by window position
    unsigned long long *bad;    // canonical: the first bad LP's batch index (all ones: none)
    double *x, *z;              // solution: the staging buffer, packed x then z by window position
};

// one LP's place in the packed layout
struct SLp {
    long long lp, toff, boff;
    int m, n;
};

// lane g of a launch over the window's tableau columns -> its LP and column jj in 0..n
template <bool RAGGED>
__device__ __forceinline__ SLp s_column(const SArgs &A, long long g, int &jj)
{
    SLp L;
    if constexpr (RAGGED) {
        const BShape *sh = A.shape;
        const long long f = A.first, base = sh[f].coff + f;     // LP i starts at coff_i + i: n_i + 1 columns each
        L.lp = plan_lane_lp(f, f + A.count, g, [=](long long i) { return sh[i].coff + i - base; });
        const BShape s = sh[L.lp];
        jj = (int)(g - (s.coff + L.lp - base));
        L.toff = s.toff;
        L.boff = s.boff;
        L.m = s.m;
        L.n = s.n;
    } else {
        const long long w = A.n + 1, k = g / w;
        jj = (int)(g - k * w);
        L.lp = A.first + k;
        L.toff = L.lp * (A.m + 1) * w;
        L.boff = L.lp * A.m;
        L.m = A.m;
        L.n = A.n;
    }
    return L;
}

// entry e of the window's packed basis -> its LP
template <bool RAGGED>
__device__ __forceinline__ long long s_entry_lp(const SArgs &A, long long e)
{
    if constexpr (RAGGED) {
        const BShape *sh = A.shape;
        const long long f = A.first, base = sh[f].boff;
        return plan_lane_lp(f, f + A.count, e, [=](long long i) { return sh[i].boff - base; });
    } else {
        return A.first + e / A.m;
    }
}

// pass 1: every row slot of the window unclaimed, every flag clear
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_canon_init(const SArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    long long b0;
    if constexpr (RAGGED) b0 = A.shape[A.first].boff;
    else b0 = A.first * A.m;
    if (g < A.nbasis) A.basis[b0 + g] = INT_MAX;
    if (g < A.count) A.flags[g] = 0;
    if (g == 0) *A.bad = ~0ull;
}

// pass 2: Tableau.isCanonical's basic columns, lanes over the tableau columns
// of the flat stack, wave s of the workgroup on constraint rows s, s + S, ...;
// a unit column of zero cost claims its row with atomicMin (the lowest column
// wins), column 0 gives flag bit 0 (some b_r < 0.0)
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_SCAN_COLS *PLAN_SCAN_MAX_SLICES) void k_canon_scan(const SArgs A)
{
    __shared__ int s_nnz[PLAN_SCAN_MAX_SLICES][PLAN_SCAN_COLS];
    __shared__ int s_one[PLAN_SCAN_MAX_SLICES][PLAN_SCAN_COLS];
    const int c = threadIdx.x & (PLAN_SCAN_COLS - 1), s = threadIdx.x / PLAN_SCAN_COLS;
    const int S = blockDim.x / PLAN_SCAN_COLS;
    const long long g = (long long)blockIdx.x * PLAN_SCAN_COLS + c;
    const bool live = g < A.lanes;
    int jj = 0, nnz = 0, one = INT_MAX;
    SLp L{};
    if (live) {
        L = s_column<RAGGED>(A, g, jj);
        const long long w = L.n + 1;
        const double *col = A.T + L.toff + w + jj;      // row 1 of the LP, this column
        if (jj == 0) {
#pragma unroll 4
            for (int i = s; i < L.m; i += S) nnz += col[i * w] < 0.0 ? 1 : 0;
        } else {
#pragma unroll 4
            for (int i = s; i < L.m; i += S) {
                const double v = col[i * w];
                nnz += v != 0.0 ? 1 : 0;                // a NaN counts
                if (v == 1.0) one = min(one, i);
            }
        }
    }
    if (S > 1) {        // uniform over the workgroup: the slices meet in LDS
        s_nnz[s][c] = nnz;
        s_one[s][c] = one;
        __syncthreads();
        if (s == 0)
            for (int k = 1; k < S; ++k) {
                nnz += s_nnz[k][c];
                one = min(one, s_one[k][c]);
            }
    }
    if (!live || s != 0) return;
    if (jj == 0) {
        if (nnz > 0) {
            atomicOr(&A.flags[L.lp - A.first], 1);
            atomicMin(A.bad, (unsigned long long)L.lp);
        }
    } else if (nnz == 1 && one != INT_MAX && A.T[L.toff + jj] == 0.0) {
        atomicMin(&A.basis[L.boff + one], jj - 1);
    }
}

// pass 3: a row nobody claimed gets -1 and gives flag bit 1
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_canon_finish(const SArgs A)
{
    const long long e = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (e >= A.nbasis) return;
    long long b0;
    if constexpr (RAGGED) b0 = A.shape[A.first].boff;
    else b0 = A.first * A.m;
    if (A.basis[b0 + e] != INT_MAX) return;
    A.basis[b0 + e] = -1;
    const long long lp = s_entry_lp<RAGGED>(A, e);
    atomicOr(&A.flags[lp - A.first], 2);
    atomicMin(A.bad, (unsigned long long)lp);
}

// Simplex.getBFS / getObjValue: lanes over the tableau columns of the flat
// stack; column 0 gives z = -T[0][0], column 1 + j gives x[j] = T[1+r][0] of the
// last row r whose basic column is j, +0.0 without one
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_solution(const SArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    int jj;
    const SLp L = s_column<RAGGED>(A, g, jj);
    const long long k = L.lp - A.first;
    if (jj == 0) {
        A.z[k] = -A.T[L.toff];
        return;
    }
    const int32_t *bs = A.basis + L.boff;
    int r = L.m - 1;
#pragma unroll 1
    for (; r >= 0; --r)
        if (bs[r] == jj - 1) break;
    // the window's columns before this one, less one column 0 per LP up to here
    A.x[g - k - 1] = r >= 0 ? A.T[L.toff + (long long)(1 + r) * (L.n + 1)] : 0.0;
}

// ---------------------------------------------------------------------------
// Problem-form batches (lp_problem_upload / lp_problem_duals).
// An LP arrives as the first ns + 1 columns of its tableau; k_assemble writes
// the window's tableaux from the staged blocks and the senses' slack table
// (batch_plan.h: plan_problem_slack), k_duals reads the duals back from row 0.
// Flat kernels as above: no workgroup reads what another writes.
// ---------------------------------------------------------------------------
struct PInfo {
    long long poff;             // LP i's problem block: doubles from the whole batch's packed blocks
    int32_t ns, pad;
};
struct FArgs {
    SArgs S;                    // the window: T, shape, first, count, nbasis, m, n; x is the duals' staging
    double *out;                // k_assemble: the packed tableaux (BArgs::T)
    const double *src;          // k_assemble: the window's staged problem blocks, packed
    const int32_t *slack;       // +(1+j) / -(1+j) / 0 per row: m entries (uniform), boff-indexed (ragged)
    const PInfo *info;          // ragged: one per LP of the batch; else null
    long long elems;            // destination elements of the window
    int ns;                     // uniform batch only
};

// lanes over the destination elements of the window's packed tableaux, each
// PLAN_ASSEMBLE_RUN consecutive ones: a staged value, +-1.0 or +0.0 by (row, column)
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_assemble(const FArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    const SArgs &S = A.S;
    const long long f = S.first;
    const double *const src = A.src;
    const int32_t *const tab = A.slack;
    auto slack = [=](long long at) { return (int)tab[at]; };
    if constexpr (RAGGED) {
        const BShape *sh = S.shape;
        const PInfo *info = A.info;
        const long long tbase = sh[f].toff, pbase = info[f].poff, hi = f + S.count;
        double *const out = A.out + tbase;
        plan_assemble_lane(
            g * PLAN_ASSEMBLE_RUN, A.elems,
            [=](long long e) { return plan_lane_lp(f, hi, e, [=](long long i) { return sh[i].toff - tbase; }); },
            [=](long long i) {
                const BShape s = sh[i];
                const PInfo p = info[i];
                return ProblemLp{s.toff - tbase, p.poff - pbase, s.boff, s.m, s.n, p.ns};
            },
            slack,
            [=](long long e, int kind, long long at) {
                out[e] = kind == PLAN_CELL_STAGED ? src[at] : kind == PLAN_CELL_PLUS ? 1.0 : kind == PLAN_CELL_MINUS ? -1.0 : 0.0;
            });
    } else {
        const int m = S.m, n = S.n, ns = A.ns;
        const long long E = (long long)(m + 1) * (n + 1), PE = (long long)(m + 1) * (ns + 1);
        double *const out = A.out + f * E;
        plan_assemble_lane(
            g * PLAN_ASSEMBLE_RUN, A.elems, [=](long long e) { return f + e / E; },
            [=](long long i) { return ProblemLp{(i - f) * E, (i - f) * PE, 0, m, n, ns}; }, slack,
            [=](long long e, int kind, long long at) {
                out[e] = kind == PLAN_CELL_STAGED ? src[at] : kind == PLAN_CELL_PLUS ? 1.0 : kind == PLAN_CELL_MINUS ? -1.0 : 0.0;
            });
    }
}

// the duals of the window's rows: lanes over its packed rows (the basis
// layout); a <= row gives -T[0][1+j], a >= row T[0][1+j], an equality the quiet NaN
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_duals(const FArgs A)
{
    const SArgs &S = A.S;
    const long long e = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (e >= S.nbasis) return;
    const long long lp = s_entry_lp<RAGGED>(S, e);
    long long toff;
    int s;
    if constexpr (RAGGED) {
        toff = S.shape[lp].toff;
        s = A.slack[S.shape[S.first].boff + e];
    } else {
        toff = lp * (long long)(S.m + 1) * (S.n + 1);
        s = A.slack[e - (lp - S.first) * S.m];
    }
    double y = __longlong_as_double(0x7ff8000000000000LL);
    if (s != 0) {
        const double c = S.T[toff + (s > 0 ? s : -s)];
        y = s > 0 ? -c : c;
    }
    S.x[e] = y;
}

// New right-hand sides on the stored tableaux (lp_resolve_set_rhs; DESIGN.md
// 4q): lanes over the (LP, row) pairs of the window, rows 0..m_i (S.lanes of
// them).  S.x is the window's staged rhs, m_i + 1 doubles per LP.  A lane
// writes T[i][0] of its own row and reads only that row's columns >= 1, the
// slack table and the staged rhs: no lane reads what another lane writes.
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_rhs(const FArgs A)
{
    const SArgs &S = A.S;
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= S.lanes) return;
    RhsAt at;
    long long toff, soff = 0;
    int m, n;
    if constexpr (RAGGED) {
        const BShape *const sh = S.shape;
        const long long f = S.first, b0 = sh[f].boff;
        at = plan_rhs_at(f, f + S.count, g, [=](long long i) { return sh[i].boff - b0 + (i - f); });
        const BShape s = sh[at.lp];
        toff = s.toff;
        soff = s.boff;
        m = s.m;
        n = s.n;
    } else {
        m = S.m;
        n = S.n;
        at = plan_rhs_at(S.first, g, m);
        toff = at.lp * (long long)(m + 1) * (n + 1);
    }
    double *const row = A.out + toff + (long long)at.row * (n + 1);
    const int32_t *const tab = A.slack + soff;
    const double *const rhs = S.x + at.base;
    row[0] = plan_rhs_cell(
        at.row, m, [=](int k) { return (int)tab[k]; }, [=](int c) { return row[c]; },
        [=](int k) { return rhs[k]; });
}

// New costs on the stored tableaux (lp_reopt_set_costs): lanes
// over the (LP, column) pairs of the window, columns 0..n_i (S.lanes of them).
// S.x is the window's staged costs, n_i + 1 doubles per LP.  A lane writes
// T[0][j] of its own column and reads only rows >= 1 of that column, the
// basis and the staged costs: no lane reads what another lane writes, and
// adjacent lanes read adjacent cells of a row.
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_cost(const FArgs A)
{
    const SArgs &S = A.S;
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= S.lanes) return;
    CostAt at;
    long long toff, boff;
    int m, n;
    if constexpr (RAGGED) {
        const BShape *const sh = S.shape;
        const long long f = S.first, c0 = sh[f].coff;
        at = plan_cost_at(f, f + S.count, g, [=](long long i) { return sh[i].coff - c0 + (i - f); });
        const BShape s = sh[at.lp];
        toff = s.toff;
        boff = s.boff;
        m = s.m;
        n = s.n;
    } else {
        m = S.m;
        n = S.n;
        at = plan_cost_at(S.first, g, n);
        toff = at.lp * (long long)(m + 1) * (n + 1);
        boff = at.lp * (long long)m;
    }
    const int w = n + 1;
    double *const T = A.out + toff;
    const double *const col = T + w + at.col;       // T[1][j]
    const int32_t *const basis = S.basis + boff;
    const double *const cost = S.x + at.base;
    T[at.col] = plan_cost_cell(
        at.col, m, n, [=](int r) { return (int)basis[r]; }, [=](int r) { return col[(long long)r * w]; },
        [=](int k) { return cost[k]; });
}

// ---------------------------------------------------------------------------
// Warm cuts (lp_cut_extend): the stored tableaux of a source
// batch with q_i more rows each, written into a destination batch.  Three flat
// kernels on the destination's stream.  Every read is of the source batch or
// of the staging, every write of the destination: no lane reads what another
// writes, and there is no atomic, fence or LDS.  Either batch may be uniform
// or ragged: the offsets come from the staged table (batch_plan.h: CutLp).
// ---------------------------------------------------------------------------
struct CArgs {
    const double *src;          // the source's packed tableaux (BArgs::T)
    const int32_t *sbasis;      // its packed basis
    double *dst;                // the destination's packed tableaux
    int32_t *dbasis;            // its packed basis
    const CutLp *lp;            // the window's table, count + 1 entries
    const double *rows;         // the staged stated rows, packed
    const int8_t *sense;        // the staged senses, packed
    long long count;            // LPs of the window
    long long lanes;            // of this launch (k_cut_copy: destination elements)
};

// The three kernels are templates defined at the end of this file and first named there
// (cut_kernel_of): a kernel is emitted where it is first named, and naming these after every other
// kernel leaves the others where they were.

// ---------------------------------------------------------------------------
// General-form batches (lp_general_*): bounds, free variables
// and maximise around the same standard-form tableaux.  Four flat kernels as
// above; the staged general blocks stay in a batch-wide buffer, each LP's at
// its own offset, so the bounds are where the recovery reads them.  The rules
// are batch_plan.h's plan_general_*, shared with the host check.
// ---------------------------------------------------------------------------
struct GArgs {
    SArgs S;                    // the window: T, shape, first, count, m = m', n = n'; x is the gathered x'
    double *out;                // the packed tableaux (BArgs::T)
    const double *stage;        // every LP's general block, packed over the whole batch
    double *shift;              // the shifted columns: m' + 1 per LP, LP i's at boff(i) + i
    const GVar *var;            // ns + nf per LP (uniform: one LP's)
    const int32_t *slack;       // m' per LP, boff-indexed (uniform: one LP's)
    const int32_t *bvar;        // likewise: the variable of a bound row
    const GInfo *info;          // ragged: one per LP of the batch; else null
    GInfo u;                    // uniform: m, ns, nf, maximise; poff the doubles of one block
    long long elems;            // destination elements of the window
    long long lanes, rows;      // of this launch; duals: the caller's rows of the window
    double *gx, *gz;            // recovery: the caller's x packed over the batch (voff), z by LP
    double *gy, *gr;            // duals: y packed over the batch (yoff), r (voff)
};
// k_general_restage's: GArgs stays as the four kernels above have it
struct GBArgs {
    GArgs G;                    // lanes: the window's border doubles
    const double *border;       // the window's staged borders, packed
    double *block;              // G.stage, to be written
};

template <bool RAGGED>
__device__ __forceinline__ GeneralLp g_lp(const GArgs &A, long long lp)
{
    GeneralLp L;
    if constexpr (RAGGED) {
        const BShape s = A.S.shape[lp];
        const GInfo g = A.info[lp];
        L = GeneralLp{s.toff, s.boff, s.coff, g.poff, g.xoff, s.boff, g.voff, g.yoff, g.m, s.m, s.n, g.ns, g.nf, g.maximise};
    } else {
        const GInfo g = A.u;
        const long long mp = A.S.m, np = A.S.n;
        L = GeneralLp{lp * (mp + 1) * (np + 1), lp * mp, lp * np, lp * g.poff, 0, 0, lp * g.ns, lp * g.m,
                      g.m, (int)mp, (int)np, g.ns, g.nf, g.maximise};
    }
    return L;
}

// lane g of a launch -> its LP of the window (plan_general_lane_lp)
template <bool RAGGED, class Start>
__device__ __forceinline__ long long g_lane_lp(const GArgs &A, long long g, long long stride, Start start, long long *rem)
{
    return plan_general_lane_lp<RAGGED>(A.S.first, A.S.count, g, stride, start, rem);
}

// the shifted column: one lane per (LP, row 0..m') of the window, each a
// sequential loop over the LP's shifted variables (plan_general_shift)
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_general_shift(const GArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const BShape *sh = A.S.shape;
    long long row;
    const long long lp = g_lane_lp<RAGGED>(A, g, A.S.m + 1, [=](long long i) { return sh[i].boff + i; }, &row);
    const GeneralLp L = g_lp<RAGGED>(A, lp);
    const GVar *var = A.var + L.xoff;
    const int bv = row > L.m ? A.bvar[L.soff + row - 1] : 0;
    A.shift[L.boff + lp + row] = plan_general_shift((int)row, L.m, L.ns, L.maximise != 0, A.stage + L.poff,
                                                    [=](int j) { return var[j]; }, bv);
}

// a new border on the stored general blocks (lp_reopt_set_general; DESIGN.md
// 4r): one lane per staged double of the window's borders, 3 ns_i + m_i + 1 per
// LP (row 0 of P, b, lb, ub), each copied to its place in the LP's block
// (plan_restage_at).  The rest of the block -- A -- stays.
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_general_restage(const GBArgs R)
{
    const GArgs &A = R.G;
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const GInfo *info = A.info;
    long long e;
    const long long lp = g_lane_lp<RAGGED>(A, g, plan_restage_border(A.u.m, A.u.ns),
                                           [=](long long i) { return 3 * info[i].voff + info[i].yoff + i; }, &e);
    const GeneralLp L = g_lp<RAGGED>(A, lp);
    R.block[L.poff + plan_restage_at(e, L.m, L.ns)] = R.border[g];
}

// lanes over the destination elements of the window's packed tableaux: a
// staged value or its flip, an entry of the shifted column, +-1.0 or +0.0
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_general_assemble(const GArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    const long long f = A.S.first;
    const BShape *sh = A.S.shape;
    const GVar *const var = A.var;
    const int32_t *const tab = A.slack;
    const double *const stage = A.stage, *const shift = A.shift;
    long long tbase, hi = f + A.S.count;
    if constexpr (RAGGED) tbase = sh[f].toff;
    else tbase = f * (long long)(A.S.m + 1) * (A.S.n + 1);
    const long long E = (long long)(A.S.m + 1) * (A.S.n + 1);
    double *const out = A.out + tbase;
    plan_general_lane(
        g, A.elems, tbase,
        [=](long long e) {
            if constexpr (RAGGED) return plan_lane_lp(f, hi, e, [=](long long i) { return sh[i].toff - tbase; });
            else return f + e / E;
        },
        [&](long long i) { return g_lp<RAGGED>(A, i); }, [=](long long at) { return var[at]; },
        [=](long long at) { return (int)tab[at]; },
        [=](long long e, int kind, long long at) {
            double v = 0.0;
            if (kind == PLAN_CELL_STAGED) v = stage[at];
            else if (kind == PLAN_CELL_STAGED_FLIP) v = plan_flip(stage[at]);
            else if (kind == PLAN_CELL_SHIFTED || kind == PLAN_CELL_RANGE) v = shift[at];
            else if (kind == PLAN_CELL_PLUS) v = 1.0;
            else if (kind == PLAN_CELL_MINUS) v = -1.0;
            out[e] = v;
        });
}

// the caller's x and objective: lanes over the window's packed caller
// variables plus one per LP, after k_solution has filled x' (A.S.x, packed
// over the window) on the same stream
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_general_recover(const GArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const GInfo *info = A.info;
    long long j;
    const long long lp = g_lane_lp<RAGGED>(A, g, A.u.ns + 1, [=](long long i) { return info[i].voff + i; }, &j);
    const GeneralLp L = g_lp<RAGGED>(A, lp);
    if (j == L.ns) {
        const double t = A.S.T[L.toff];
        A.gz[lp] = L.maximise ? t : -t;
        return;
    }
    long long c0;
    if constexpr (RAGGED) c0 = A.S.shape[A.S.first].coff;
    else c0 = A.S.first * (long long)A.S.n;
    const double *xp = A.S.x + (L.coff - c0);
    const GVar v = A.var[L.xoff + j];
    const double *lb = A.stage + L.poff + (long long)(L.m + 1) * (L.ns + 1), *ub = lb + L.ns;
    const int k = v.kind;
    A.gx[L.voff + j] = plan_general_x(k, xp[j], k == PLAN_VAR_FREE ? xp[v.neg - 1] : 0.0,
                                      k == PLAN_VAR_LOWER || k == PLAN_VAR_BOXED ? lb[j] : 0.0,
                                      k == PLAN_VAR_UPPER ? ub[j] : 0.0);
}

// the caller's duals and reduced costs from row 0 of the stored tableaux:
// lanes [0, rows) over the window's packed caller rows, the rest over its
// packed caller variables
template <bool RAGGED>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_general_duals(const GArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const GInfo *info = A.info;
    long long at;
    if (g < A.rows) {
        const long long lp = g_lane_lp<RAGGED>(A, g, A.u.m, [=](long long i) { return info[i].yoff; }, &at);
        const GeneralLp L = g_lp<RAGGED>(A, lp);
        const int s = A.slack[L.soff + at];
        double y = __longlong_as_double(0x7ff8000000000000LL);
        if (s != 0) y = plan_general_y(s, A.S.T[L.toff + (s > 0 ? s : -s)], L.maximise != 0);
        A.gy[L.yoff + at] = y;
        return;
    }
    const long long lp = g_lane_lp<RAGGED>(A, g - A.rows, A.u.ns, [=](long long i) { return info[i].voff; }, &at);
    const GeneralLp L = g_lp<RAGGED>(A, lp);
    const GVar v = A.var[L.xoff + at];
    const double *row0 = A.S.T + L.toff;
    // a bound row is a <= row: its slack entry is the tableau column itself
    const double cb = v.kind == PLAN_VAR_BOXED ? row0[A.slack[L.soff + v.brow - 1]] : 0.0;
    A.gr[L.voff + at] = plan_general_r(v.kind, row0[1 + at], cb, L.maximise != 0);
}

}  // namespace
}  // namespace lpk

using lpk::BArgs;
using lpk::BRec;
using lpk::TArgs;
using lpk::TRec;

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct lp_batch {
    int dev = 0;
    hipStream_t s = nullptr;
    int64_t count = 0, m = 0, n = 0, logcap = 0, chunk = 4096;
    int pitch = 0, waves = 1;
    size_t lds = 0;
    // placement (lp_placed_create): what was asked for, and what each LP
    // got -- one flag on a uniform batch, one per LP on a ragged one
    int place = LP_PLACE_LDS;
    bool on_device = false;
    std::vector<uint8_t> lp_on_device;
    bool any_on_device = false;
    // teams (lp_teamed_create): the request, what each LP got, and for the LPs with a
    // team above 1 the workgroup table, the second tableau buffer and the second record array
    std::vector<int32_t> team_req;              // per LP: 0 auto, 1, or G (empty: every LP 1)
    std::vector<int32_t> team;                  // per LP, >= 1 (empty: no LP is teamed)
    std::vector<lpk::TeamWG> hwg;
    lpk::TeamWG *wg = nullptr;
    double *T2 = nullptr;
    BRec *rec2 = nullptr;
    std::vector<BRec> hrec_team;
    size_t team_lds = 0;                        // the largest plan_device_lds among the teamed LPs
    int64_t window = LPK_TEAM_WINDOW;           // launches of k_batch_team per read-back of the records
    double *T = nullptr;
    BRec *rec = nullptr;
    long long *log = nullptr;
    int32_t *basis = nullptr;
    bool basis_on = false;
    lp_tol tol{};
    std::vector<BRec> hrec;
    // two-phase state, allocated by the first lp_twophase_solve
    double *W = nullptr, *origc = nullptr;
    TRec *trec = nullptr;
    std::vector<TRec> htrec;
    std::vector<int64_t> nlog;      // pivots logged per LP by the last two-phase call (else empty)
    // ragged batch (lp_ragged_create): m, n, pitch, waves and lds above are unused
    bool ragged = false;
    std::vector<lpk::BShape> hshape;            // count (ragged only)
    lpk::BShape *shape = nullptr;               // its device copy, written once at create
    double *zbuf = nullptr;                     // count: lp_batch_objective's gather
    // batch solutions, each allocated by the first call that needs it
    double *sol = nullptr;                      // lp_solution_gather's staging: x packed (coff(count)), then z (count)
    unsigned long long *canon = nullptr;        // lp_solution_canonical's: the first bad LP, then the flags (count int32)
    // problem form: the senses' slack table and, on a ragged batch, each LP's problem
    // block, set by lp_problem_set_senses; the two staging buffers by the first call that needs them
    bool senses_on = false;
    std::vector<lpk::PInfo> hinfo;              // count + 1 (both kinds): poff and ns per LP, the total last
    int32_t *slack = nullptr;                   // m entries (uniform) or boff(count) (ragged)
    lpk::PInfo *pinfo = nullptr;                // count (ragged only)
    double *pstage = nullptr;                   // lp_problem_upload's staging, pstage_cap doubles
    int64_t pstage_cap = 0;
    double *dual = nullptr;                     // lp_problem_duals' staging: boff(count) doubles
    // warm re-solves: the senses' table once more on the host, to name an equality row;
    // lp_resolve_set_rhs' staging; and the LPs whose last two-phase call left fewer than m live rows
    std::vector<int32_t> hslack;                // as `slack`
    double *rhs = nullptr;                      // boff(count) + count doubles
    std::vector<uint8_t> short_rows;            // per LP (empty: none), cleared by an upload
    // general form, set by lp_general_set_form: the per-LP tables, and the buffers the
    // first call that needs them allocates (a new form frees them: their sizes follow it)
    bool form_on = false;
    std::vector<lpk::GInfo> hg;                 // count + 1 (both kinds): offsets and counts per LP, the totals last
    lpk::GVar *gvar = nullptr;                  // xoff(count) entries (uniform: ns + nf)
    int32_t *gslack = nullptr, *gbvar = nullptr;    // boff(count) entries each (uniform: m')
    lpk::GInfo *ginfo = nullptr;                // count (ragged only)
    double *gstage = nullptr;                   // every LP's general block at its poff: the bounds stay here
    double *gshift = nullptr;                   // boff(count) + count: the shifted columns
    double *gsol = nullptr;                     // voff(count) + count: the caller's x, then z
    double *gdual = nullptr;                    // yoff(count) + voff(count): y, then r
    // warm re-optimisation: lp_reopt_set_costs' staging; the form's var and slack tables
    // once more on the host, to check a new border against the kinds and to name an equality row; and
    // lp_reopt_set_general's staging (freed with the form's buffers: its size follows the form)
    double *cost = nullptr;                     // coff(count) + count doubles
    std::vector<lpk::GVar> hgvar;               // as `gvar`
    std::vector<int32_t> hgslack;               // as `gslack`
    double *gborder = nullptr;                  // 3 voff(count) + yoff(count) + count doubles
    // warm cuts, on the destination of lp_cut_extend: the staged rows, and the window's
    // table followed by the senses; each grows to the largest call so far
    double *cutrows = nullptr;
    int64_t cutrows_cap = 0;                    // doubles
    unsigned char *cuttab = nullptr;
    int64_t cuttab_cap = 0;                     // bytes
    // the launch plans, plain [0], two-phase [1] and phased [2]; a uniform batch plans one bin
    lpk::BatchPlan plan[3];
    bool planned[3] = {false, false, false};
    int32_t *order[3] = {nullptr, nullptr, nullptr};    // the bins' order arrays back to back (ragged only)
    bool tp_attr = false;       // uniform batch: k_twophase's dynamic LDS was granted and set
    std::string err;

    // packed layout, both kinds: LP i's tableau, basis, two-phase working tableau and saved costs
    int64_t lp_m(int64_t i) const { return ragged ? hshape[(size_t)i].m : m; }
    int64_t lp_n(int64_t i) const { return ragged ? hshape[(size_t)i].n : n; }
    bool lp_dev(int64_t i) const { return ragged ? lp_on_device[(size_t)i] != 0 : on_device; }
    int64_t toff(int64_t i) const
    {
        if (!ragged) return i * (m + 1) * (n + 1);
        return i < count ? hshape[(size_t)i].toff : hshape.back().toff + (lp_m(count - 1) + 1) * (lp_n(count - 1) + 1);
    }
    int64_t boff(int64_t i) const
    {
        if (!ragged) return i * m;
        return i < count ? hshape[(size_t)i].boff : hshape.back().boff + lp_m(count - 1);
    }
    int64_t woff(int64_t i) const
    {
        if (!ragged) return i * (m + 1) * (n + 1 + m);
        const int64_t l = count - 1;
        return i < count ? hshape[(size_t)i].woff : hshape.back().woff + (lp_m(l) + 1) * (lp_n(l) + 1 + lp_m(l));
    }
    int64_t coff(int64_t i) const
    {
        if (!ragged) return i * n;
        return i < count ? hshape[(size_t)i].coff : hshape.back().coff + lp_n(count - 1);
    }
};

static std::string g_batch_err;

constexpr size_t BATCH_LDS_MAX = 160u * 1024u;      // one CU's LDS
// (m+1)(n+1) up to here: one wave per LP, four above (DESIGN.md "Batched solve";
// the A/B builds of scripts/batch_waves.py move it with -DLPGPU_BATCH_ONE_WAVE_ELEMS=)
#ifndef LPGPU_BATCH_ONE_WAVE_ELEMS
#define LPGPU_BATCH_ONE_WAVE_ELEMS 2048
#endif
constexpr int64_t BATCH_ONE_WAVE_ELEMS = LPGPU_BATCH_ONE_WAVE_ELEMS;
// waves per device-placed LP: 4, 8 or 16, picked by measurement (DESIGN.md 4j;
// the A/B builds of scripts/place_waves.py move it with -DLPK_BATCH_DEV_WAVES=)
#ifndef LPK_BATCH_DEV_WAVES
#define LPK_BATCH_DEV_WAVES 16
#endif
constexpr int BATCH_DEV_WAVES = LPK_BATCH_DEV_WAVES;
static_assert(BATCH_DEV_WAVES == 4 || BATCH_DEV_WAVES == 8 || BATCH_DEV_WAVES == 16, "waves per device-placed LP");
// waves per device-placed LP of the two-phase call: 8 or 16, picked by
// measurement (the A/B builds of scripts/phased_waves.py move it
// with -DLPK_PHASED_WAVES=)
#ifndef LPK_PHASED_WAVES
#define LPK_PHASED_WAVES 16
#endif
constexpr int PHASED_WAVES = LPK_PHASED_WAVES;
static_assert(PHASED_WAVES == 8 || PHASED_WAVES == 16, "waves per device-placed two-phase LP");
// element updates one launch applies per device-placed LP at the most: a
// workgroup alone on a CU was measured at 1.4e9 or more of them per second
// (profiles/r10/place_waves.json), so a launch stays below about 24 ms, twice
// that where a CU holds two LPs
#ifndef LPK_BATCH_DEV_WORK
#define LPK_BATCH_DEV_WORK (32LL << 20)
#endif
constexpr int64_t BATCH_DEV_WORK = LPK_BATCH_DEV_WORK;
// the teamed batch's knobs (knobs.h; the A/B builds of scripts/team_sweep.py)
constexpr int TEAM_WAVES = LPK_TEAM_WAVES;
static_assert(TEAM_WAVES == 4 || TEAM_WAVES == 8 || TEAM_WAVES == 16, "waves per workgroup of a team");
constexpr int TEAM_MAX = LPK_TEAM_MAX;
constexpr int64_t TEAM_MIN_ELEMS = LPK_TEAM_MIN_ELEMS;
constexpr int64_t TEAM_LP_ELEMS = LPK_TEAM_LP_ELEMS;
static_assert(TEAM_MAX >= 1 && TEAM_MIN_ELEMS >= 2 && LPK_TEAM_WINDOW >= 1, "team knobs");
static_assert(lpk::PLAN_PLACE_LDS == LP_PLACE_LDS && lpk::PLAN_PLACE_AUTO == LP_PLACE_AUTO &&
                  lpk::PLAN_PLACE_DEVICE == LP_PLACE_DEVICE,
              "batch_plan.h mirrors LP_PLACE_*");

#define BCHK(b, expr)                                                              \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) {                                                    \
            (b)->err = std::string(#expr) + ": " + hipGetErrorString(e_);          \
            /* reported here: the runtime keeps it as the thread's last error   */ \
            /* until read, and a later launch's hipGetLastError() would find it */ \
            (void)hipGetLastError();                                               \
            return LP_DEVICE_ERROR;                                                \
        }                                                                          \
    } while (0)

static int bfail(lp_batch *b, const char *msg)
{
    b->err = msg;
    return LP_BAD_ARG;
}

// ---- the solve kernels: one table, one launcher, one place that asks the device for dynamic LDS
// k_batch, k_batch_dev, k_batch_team (and its k_team_home), k_twophase, k_twophase_dev
enum KFamily { K_PLAIN, K_DEVICE, K_TEAM, K_TEAM_HOME, K_TWOPHASE, K_PHASED };

// waves: 1 or 4, for K_PLAIN and K_TWOPHASE (the other families have one width each);
// maxinc: the LP_RULE_MAX_INCREASE instantiation, K_PLAIN and K_DEVICE only;
// dual: the LP_RULE_DUAL instantiation, likewise
struct KKey {
    KFamily family;
    bool ragged;
    int waves = 1;
    bool maxinc = false;
    bool dual = false;
};

static int kernel_waves(const KKey &k)
{
    switch (k.family) {
    case K_DEVICE: return BATCH_DEV_WAVES;
    case K_TEAM: return TEAM_WAVES;
    case K_TEAM_HOME: return 4;
    case K_PHASED: return PHASED_WAVES;
    default: return k.waves == 1 ? 1 : 4;
    }
}

// The max-increase instantiations, defined at the end of this file: a kernel is emitted where it
// is first named, and naming these after every other kernel leaves the others where they were.
static const void *maxinc_kernel_of(const KKey &k);
// The dual rule's, after those: the same reason.
static const void *dual_kernel_of(const KKey &k);

// (u = 1 for a uniform batch: DEVICE, PHASED and TEAM name the ragged instantiation first, the
// order these kernels have always been emitted in)
static const void *kernel_of(const KKey &k)
{
    using namespace lpk;
    if (k.maxinc) return maxinc_kernel_of(k);
    if (k.dual) return dual_kernel_of(k);
    const int r = k.ragged ? 1 : 0, u = 1 - r, w = k.waves == 1 ? 0 : 1;
    static const void *const PLAIN[2][2] = {         // [ragged][four waves]
        {(const void *)&k_batch<1>, (const void *)&k_batch<4>},
        {(const void *)&k_batch<1, true>, (const void *)&k_batch<4, true>}};
    static const void *const TWOPHASE[2][2] = {      // [ragged][four waves]
        {(const void *)&k_twophase<1>, (const void *)&k_twophase<4>},
        {(const void *)&k_twophase<1, true>, (const void *)&k_twophase<4, true>}};
    static const void *const DEVICE[2] = {(const void *)&k_batch_dev<BATCH_DEV_WAVES, true>,
                                          (const void *)&k_batch_dev<BATCH_DEV_WAVES>};
    static const void *const PHASED[2] = {(const void *)&k_twophase_dev<PHASED_WAVES, true>,
                                          (const void *)&k_twophase_dev<PHASED_WAVES>};
    static const void *const TEAM[2] = {(const void *)&k_batch_team<TEAM_WAVES, true>,
                                        (const void *)&k_batch_team<TEAM_WAVES>};
    static const void *const HOME[2] = {(const void *)&k_team_home<true>, (const void *)&k_team_home<false>};
    switch (k.family) {
    case K_PLAIN: return PLAIN[r][w];
    case K_DEVICE: return DEVICE[u];
    case K_TEAM: return TEAM[u];
    case K_TEAM_HOME: return HOME[u];
    case K_TWOPHASE: return TWOPHASE[r][w];
    default: return PHASED[u];
    }
}

// args: the kernel's one parameter.  The caller reads hipGetLastError().
static void launch(const KKey &k, dim3 grid, size_t lds, hipStream_t s, void *args)
{
    void *kargs[1] = {args};
    (void)hipLaunchKernel(kernel_of(k), grid, dim3(64 * kernel_waves(k)), kargs, lds, s);
}

// what one workgroup may ask for on this device
static int lds_granted(lp_batch *b, int *granted)
{
    BCHK(b, hipDeviceGetAttribute(granted, hipDeviceAttributeMaxSharedMemoryPerBlock, b->dev));
    return LP_PIVOTED;
}

// the figures every refusal below carries
static std::string lds_needs(int64_t lds, int granted)
{
    return ": needs " + std::to_string(lds) + " bytes of LDS per workgroup, the device grants " + std::to_string(granted);
}

// The dynamic LDS of kernel k against the device's grant: above it the call is refused with
// `refusal`; above 64 KiB it becomes the kernel's attribute, and that of its max-increase and dual
// twins (K_PLAIN and K_DEVICE: the plain call's kernels, the only ones that have them).
static int lds_grant(lp_batch *b, int granted, const KKey &k, int64_t lds, const std::string &refusal)
{
    if (lds > (int64_t)granted) {
        b->err = refusal;
        return LP_BAD_ARG;
    }
    if (lds <= 64 * 1024) return LP_PIVOTED;
    BCHK(b, hipFuncSetAttribute(kernel_of(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (k.family == K_PLAIN || k.family == K_DEVICE) {
        KKey x = k;
        x.maxinc = true;
        BCHK(b, hipFuncSetAttribute(kernel_of(x), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        x.maxinc = false;
        x.dual = true;
        BCHK(b, hipFuncSetAttribute(kernel_of(x), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    return LP_PIVOTED;
}

static const char *const PHASED_TOO_LARGE =
    "too large for the two-phase batch path in device memory: the pivot row, the multipliers, the reduction "
    "scratch and the basis, (n+1+m) + (m+1) + 16 + (m+1)/2 float64, must fit one CU's 160 KiB of LDS "
    "(use Simplex per LP)";

// The launch plan of the plain (0), the two-phase (1) or the phased (2) call,
// made once per batch (batch_plan.h).  An LP too large for a CU is refused
// before any device call; then the workgroups a CU holds by wave slots and
// registers come from the runtime at zero dynamic LDS, and a ragged batch's
// order arrays go to the device, bin after bin.
static int ensure_plan(lp_batch *b, int tp)
{
    if (b->planned[tp]) return LP_PIVOTED;
    const size_t cnt = (size_t)b->count;
    std::vector<int64_t> ms(cnt), ns(cnt);
    bool phased_dev = false;
    for (size_t i = 0; i < cnt; ++i) {
        ms[i] = b->lp_m((int64_t)i);
        ns[i] = b->lp_n((int64_t)i);
        if (tp == 0 && b->lp_dev((int64_t)i)) continue;         // its side buffers were checked at create
        if (tp == 2 && b->place != LP_PLACE_LDS) {              // an LDS batch: the two-phase test below
            const int where = lpk::plan_place_phased(b->place, ms[i], ns[i]);
            if (where < 0) {
                b->err = "LP " + std::to_string(i) + " (" + std::to_string(ms[i]) + " x " + std::to_string(ns[i]) +
                         ") is " + PHASED_TOO_LARGE;
                return LP_BAD_ARG;
            }
            phased_dev = phased_dev || where == lpk::PLAN_PLACE_DEVICE;
            continue;
        }
        if (lpk::plan_need(tp != 0, ms[i], ns[i]) > lpk::PLAN_LDS_MAX) {
            b->err = "LP " + std::to_string(i) + " (" + std::to_string(ms[i]) + " x " + std::to_string(ns[i]) +
                     ") is too large for the " + (tp ? "two-phase " : "") +
                     "batch path: its tableau and side buffers must fit one CU's 160 KiB of LDS";
            return LP_BAD_ARG;
        }
    }
    BCHK(b, hipSetDevice(b->dev));
    int cap[2] = {0, 0};
    for (int w = 0; w < 2; ++w)
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &cap[w], kernel_of({tp ? K_TWOPHASE : K_PLAIN, b->ragged, w ? 4 : 1}), w ? 256 : 64, 0));
    int dev_cap = 0;
    if (tp == 0 && b->any_on_device)
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&dev_cap, kernel_of({K_DEVICE, b->ragged}),
                                                             64 * BATCH_DEV_WAVES, 0));
    if (phased_dev)
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&dev_cap, kernel_of({K_PHASED, b->ragged}),
                                                             64 * PHASED_WAVES, 0));
    // the plain call's plan leaves out the LPs a team works on (k_batch_team launches them)
    const bool sub = tp == 0 && !b->hwg.empty();
    std::vector<int32_t> solo;
    if (sub) {
        for (size_t i = 0; i < cnt; ++i)
            if (b->team[i] <= 1) {
                ms[solo.size()] = ms[i];
                ns[solo.size()] = ns[i];
                solo.push_back((int32_t)i);
            }
    }
    const int64_t nplan = sub ? (int64_t)solo.size() : b->count;
    lpk::BatchPlan P =
        tp == 0 && b->any_on_device
            ? lpk::plan_placed(nplan, ms.data(), ns.data(), b->place, cap[0], cap[1], BATCH_ONE_WAVE_ELEMS,
                               BATCH_DEV_WAVES, dev_cap)
        : phased_dev
            ? lpk::plan_phased(b->count, ms.data(), ns.data(), b->place, cap[0], cap[1], BATCH_ONE_WAVE_ELEMS,
                               PHASED_WAVES, dev_cap)
            : lpk::plan_ragged(nplan, ms.data(), ns.data(), tp != 0, cap[0], cap[1], BATCH_ONE_WAVE_ELEMS);
    if (sub)
        for (lpk::PlanBin &bin : P.bins)
            for (int32_t &i : bin.order) i = solo[(size_t)i];
    // Every bin against the device's grant, in plan order.  A device bin (the plain call's plan
    // and the phased one have them, the two-phase plan has none) sets its kernel's attribute; the
    // LDS bins of a ragged batch set the largest of each width class, once, below.
    int granted = 0;
    {
        const int st = lds_granted(b, &granted);
        if (st != LP_PIVOTED) return st;
    }
    const KFamily lds_family = tp ? K_TWOPHASE : K_PLAIN;
    int64_t most[2] = {0, 0};
    for (const lpk::PlanBin &bin : P.bins) {
        const std::string refusal = "LP " + std::to_string(bin.order[0]) +
                                    " is too large for the batch path on this device" + lds_needs(bin.lds, granted);
        if (bin.device) {
            const int st = lds_grant(b, granted, {tp == 2 ? K_PHASED : K_DEVICE, b->ragged}, bin.lds, refusal);
            if (st != LP_PIVOTED) return st;
            continue;
        }
        if (bin.lds > (int64_t)granted) {
            b->err = refusal;
            return LP_BAD_ARG;
        }
        int64_t &mx = most[bin.waves == 1 ? 0 : 1];
        mx = std::max(mx, bin.lds);
    }
    if (b->ragged) {
        for (int w = 0; w < 2; ++w) {
            const int st = lds_grant(b, granted, {lds_family, true, w ? 4 : 1}, most[w], "");     // (checked above)
            if (st != LP_PIVOTED) return st;
        }
        std::vector<int32_t> all;
        all.reserve(cnt);
        for (const lpk::PlanBin &bin : P.bins) all.insert(all.end(), bin.order.begin(), bin.order.end());
        if (!b->order[tp]) BCHK(b, hipMalloc(&b->order[tp], cnt * sizeof(int32_t)));
        if (!all.empty()) {
            BCHK(b, hipMemcpyAsync(b->order[tp], all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                   b->s));
            BCHK(b, hipStreamSynchronize(b->s));
        }
    }
    b->plan[tp] = std::move(P);
    b->planned[tp] = true;
    return LP_PIVOTED;
}

static bool bin_unfinished(const lp_batch *b, const lpk::PlanBin &bin)
{
    for (const int32_t i : bin.order)
        if (b->hrec[(size_t)i].state != lpk::B_DONE) return true;
    return false;
}

// The teams of a batch made by lp_teamed_create (batch_plan.h).  Forced teams
// were checked before any device call; an auto request needs the runtime's
// answer for `slots`.  Where an LP gets a team above 1, the workgroup table
// goes to the device and the second buffer and record array are allocated.
static int team_setup(lp_batch *b)
{
    const size_t cnt = (size_t)b->count;
    bool any = false, any_auto = false;
    int64_t n_dev = 0;
    for (size_t i = 0; i < b->team_req.size(); ++i) {
        any = any || b->team_req[i] != 1;
        any_auto = any_auto || (b->team_req[i] == 0 && b->lp_dev((int64_t)i));
        n_dev += b->lp_dev((int64_t)i) ? 1 : 0;
    }
    if (!any) return LP_PIVOTED;
    int64_t slots = 0;
    if (any_auto) {
        int per_cu = 0, cus = 0;
        BCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_of({K_TEAM, b->ragged}), 64 * TEAM_WAVES,
                                                             0));
        BCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->dev));
        slots = (int64_t)std::max(1, per_cu) * cus;
    }
    b->team.assign(cnt, 1);
    std::vector<int64_t> ms(cnt), ns(cnt), to(cnt);
    for (size_t i = 0; i < cnt; ++i) {
        ms[i] = b->lp_m((int64_t)i);
        ns[i] = b->lp_n((int64_t)i);
        to[i] = b->toff((int64_t)i);
        if (!b->lp_dev((int64_t)i)) continue;       // an LDS-placed LP has no team
        const int g = lpk::plan_team_size(b->team_req[i], n_dev, ms[i], ns[i], slots, TEAM_MAX, TEAM_MIN_ELEMS,
                                             TEAM_LP_ELEMS);
        if (g < 1) return bfail(b, "team refused");  // (forced teams were checked at create)
        b->team[i] = g;
        if (g > 1) b->team_lds = std::max(b->team_lds, (size_t)lpk::plan_device_lds(ms[i], ns[i]));
    }
    b->hwg = lpk::plan_team_table(b->count, ms.data(), ns.data(), to.data(), b->team.data());
    if (b->hwg.empty()) return LP_PIVOTED;
    int granted = 0;
    int st = lds_granted(b, &granted);
    if (st == LP_PIVOTED)
        st = lds_grant(b, granted, {K_TEAM, b->ragged}, (int64_t)b->team_lds,
                       "a teamed LP is too large for the batch path on this device");
    if (st != LP_PIVOTED) return st;
    const size_t wbytes = b->hwg.size() * sizeof(lpk::TeamWG), elems = (size_t)b->toff(b->count);
    BCHK(b, hipMalloc(&b->wg, wbytes));
    BCHK(b, hipMemcpyAsync(b->wg, b->hwg.data(), wbytes, hipMemcpyHostToDevice, b->s));
    BCHK(b, hipMalloc(&b->T2, elems * sizeof(double)));
    BCHK(b, hipMemsetAsync(b->T2, 0, elems * sizeof(double), b->s));
    BCHK(b, hipMalloc(&b->rec2, cnt * sizeof(BRec)));
    BCHK(b, hipMemsetAsync(b->rec2, 0, cnt * sizeof(BRec), b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

static int batch_alloc(lp_batch *b)
{
    BCHK(b, hipSetDevice(b->dev));
    if (!b->ragged) {
        int granted = 0;
        int st = lds_granted(b, &granted);
        if (st == LP_PIVOTED)
            st = lds_grant(b, granted, {b->on_device ? K_DEVICE : K_PLAIN, false, b->waves}, (int64_t)b->lds,
                           "shape too large for the batch path on this device" + lds_needs((int64_t)b->lds, granted) +
                               " (use lp_create)");
        if (st != LP_PIVOTED) return st;
    }
    BCHK(b, hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking));
    if (b->ragged) {
        const size_t sbytes = (size_t)b->count * sizeof(lpk::BShape);
        BCHK(b, hipMalloc(&b->shape, sbytes));
        BCHK(b, hipMemcpyAsync(b->shape, b->hshape.data(), sbytes, hipMemcpyHostToDevice, b->s));
    }
    if (!b->team_req.empty()) {     // before the plan: it leaves the teamed LPs out
        const int st = team_setup(b);
        if (st != LP_PIVOTED) return st;
    }
    if (b->ragged) {
        const int st = ensure_plan(b, 0);
        if (st != LP_PIVOTED) return st;
    }
    const size_t elems = (size_t)b->toff(b->count);
    BCHK(b, hipMalloc(&b->T, elems * sizeof(double)));
    BCHK(b, hipMemsetAsync(b->T, 0, elems * sizeof(double), b->s));
    BCHK(b, hipMalloc(&b->rec, (size_t)b->count * sizeof(BRec)));
    BCHK(b, hipMemsetAsync(b->rec, 0, (size_t)b->count * sizeof(BRec), b->s));
    if (b->logcap > 0)
        BCHK(b, hipMalloc(&b->log, (size_t)b->count * (size_t)b->logcap * 2 * sizeof(long long)));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

extern "C" int lp_batch_destroy(lp_batch *b)
{
    if (!b) return LP_BAD_ARG;
    if (b->s || b->T || b->rec || b->log || b->basis || b->W || b->origc || b->trec || b->shape) {
        (void)hipSetDevice(b->dev);
        if (b->s) (void)hipStreamSynchronize(b->s);
        if (b->shape) (void)hipFree(b->shape);
        if (b->zbuf) (void)hipFree(b->zbuf);
        if (b->sol) (void)hipFree(b->sol);
        if (b->canon) (void)hipFree(b->canon);
        if (b->slack) (void)hipFree(b->slack);
        if (b->pinfo) (void)hipFree(b->pinfo);
        if (b->pstage) (void)hipFree(b->pstage);
        if (b->dual) (void)hipFree(b->dual);
        if (b->rhs) (void)hipFree(b->rhs);
        if (b->cost) (void)hipFree(b->cost);
        if (b->cutrows) (void)hipFree(b->cutrows);
        if (b->cuttab) (void)hipFree(b->cuttab);
        for (void *p : {(void *)b->gvar, (void *)b->gslack, (void *)b->gbvar, (void *)b->ginfo, (void *)b->gstage,
                        (void *)b->gshift, (void *)b->gsol, (void *)b->gdual, (void *)b->gborder})
            if (p) (void)hipFree(p);
        if (b->wg) (void)hipFree(b->wg);
        if (b->T2) (void)hipFree(b->T2);
        if (b->rec2) (void)hipFree(b->rec2);
        if (b->order[0]) (void)hipFree(b->order[0]);
        if (b->order[1]) (void)hipFree(b->order[1]);
        if (b->order[2]) (void)hipFree(b->order[2]);
        if (b->T) (void)hipFree(b->T);
        if (b->rec) (void)hipFree(b->rec);
        if (b->log) (void)hipFree(b->log);
        if (b->basis) (void)hipFree(b->basis);
        if (b->W) (void)hipFree(b->W);
        if (b->origc) (void)hipFree(b->origc);
        if (b->trec) (void)hipFree(b->trec);
        if (b->s) (void)hipStreamDestroy(b->s);
    }
    delete b;
    return LP_PIVOTED;
}

extern "C" int64_t lp_placed_lds_bytes(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0) return LP_BAD_ARG;
    return lpk::plan_device_lds(m, n);
}

extern "C" int lp_placed_placement(const lp_batch *b, int64_t index, int *place)
{
    if (!b || !place) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    *place = b->lp_dev(index) ? LP_PLACE_DEVICE : LP_PLACE_LDS;
    return LP_PIVOTED;
}

extern "C" int lp_teamed_size(const lp_batch *b, int64_t index, int *team)
{
    if (!b || !team) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    *team = b->team.empty() ? 1 : b->team[(size_t)index];
    return LP_PIVOTED;
}

// the workgroup table, one row of five per workgroup
extern "C" int lp_teamed_plan(lp_batch *b, int64_t *rows, int64_t cap, int64_t *count)
{
    if (!b) return LP_BAD_ARG;
    if (cap < 0 || (cap > 0 && !rows)) return bfail(b, "bad rows buffer");
    if (count) *count = (int64_t)b->hwg.size();
    for (size_t k = 0; k < b->hwg.size() && (int64_t)k < cap; ++k) {
        const lpk::TeamWG &w = b->hwg[k];
        rows[5 * k] = w.lp;
        rows[5 * k + 1] = w.rank;
        rows[5 * k + 2] = w.G;
        rows[5 * k + 3] = w.e0;
        rows[5 * k + 4] = w.e1;
    }
    return LP_PIVOTED;
}

extern "C" int lp_teamed_set_window(lp_batch *b, int64_t launches_per_readback)
{
    if (!b) return LP_BAD_ARG;
    if (launches_per_readback < 1) return bfail(b, "launches_per_readback must be >= 1");
    b->window = launches_per_readback;
    return LP_PIVOTED;
}

static const char *const DEV_TOO_LARGE =
    "too large for the batch path in device memory: the pivot row, the multipliers and the reduction "
    "scratch, (n+1) + (m+1) + 16 float64, must fit one CU's 160 KiB of LDS (use lp_create)";

static const char *const TEAM_NEEDS_DEVICE =
    "a team above 1 needs a device-placed LP: LP_PLACE_AUTO or LP_PLACE_DEVICE, not LP_PLACE_LDS";

// why plan_team_size refuses request `team` for an m x n LP ("": it does not)
static std::string team_refusal(int team, int64_t m, int64_t n)
{
    if (team < 0) return "team must be 0 (auto), 1 or the number of workgroups per LP";
    if (team > TEAM_MAX) return "team " + std::to_string(team) + " is above the largest team, " + std::to_string(TEAM_MAX);
    if (lpk::plan_team_size(team, 1, m, n, 0, TEAM_MAX, TEAM_MIN_ELEMS) < 0)
        return "team " + std::to_string(team) + " is above (m+1)(n+1) / 2 of the " + std::to_string(m) + " x " +
               std::to_string(n) + " LP: every workgroup of a team needs a pair of elements";
    return "";
}

// lp_placed_create with a team request (lp_teamed_create); team 1 is lp_placed_create itself
static int create_uniform(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, int place, int team,
                          lp_batch **out)
{
    if (!out) {
        g_batch_err = "out is NULL";
        return LP_BAD_ARG;
    }
    *out = nullptr;
    if (place != LP_PLACE_LDS && place != LP_PLACE_AUTO && place != LP_PLACE_DEVICE) {
        g_batch_err = "unknown place: LP_PLACE_LDS, LP_PLACE_AUTO or LP_PLACE_DEVICE";
        return LP_BAD_ARG;
    }
    if (count <= 0 || m <= 0 || n <= 0 || log_cap < 0) {
        g_batch_err = "need count > 0, m > 0, n > 0 and log_cap >= 0";
        return LP_BAD_ARG;
    }
    if (team != 1) {
        if (team > 1 && place == LP_PLACE_LDS) {
            g_batch_err = TEAM_NEEDS_DEVICE;
            return LP_BAD_ARG;
        }
        if (m < (1 << 20) && n < (1 << 20)) g_batch_err = team_refusal(team, m, n);
        else g_batch_err.clear();       // (refused "too large" below)
        if (!g_batch_err.empty()) return LP_BAD_ARG;
    }
    // (m+1) rows at an odd pitch + P (pitch) + F (m+1) + 16 of scratch, in doubles
    const int64_t pitch = (n + 1) | 1;
    const bool small = m < (1 << 20) && n < (1 << 20);
    int64_t need = small ? ((m + 1) * pitch + pitch + (m + 1) + 16) * 8 : INT64_MAX;
    // a teamed LP is always device-placed
    const bool on_device = place == LP_PLACE_DEVICE || team > 1 ||
                           (place == LP_PLACE_AUTO && need > (int64_t)BATCH_LDS_MAX);
    if (on_device) {
        need = lpk::plan_device_lds(m, n);
        if (need > (int64_t)BATCH_LDS_MAX) {
            g_batch_err = std::string("shape ") + DEV_TOO_LARGE;
            return LP_BAD_ARG;
        }
    } else if (need > (int64_t)BATCH_LDS_MAX) {
        g_batch_err = "shape too large for the batch path: (m+1) x (n+1) float64 plus its side "
                      "buffers must fit one CU's 160 KiB of LDS (use lp_create)";
        return LP_BAD_ARG;
    }
    if (count > INT_MAX || log_cap > (INT64_MAX >> 5) / count) {
        g_batch_err = "batch too large: count or count x log_cap out of range";
        return LP_BAD_ARG;
    }
    lp_batch *b = new lp_batch;
    b->dev = device;
    b->count = count;
    b->m = m;
    b->n = n;
    b->logcap = log_cap;
    b->pitch = (int)pitch;
    b->lds = (size_t)need;
    b->place = place;
    b->on_device = b->any_on_device = on_device;
    b->waves = (m + 1) * (n + 1) <= BATCH_ONE_WAVE_ELEMS ? 1 : 4;
    if (team != 1) b->team_req.assign((size_t)count, team);
    lp_default_tol(&b->tol);
    b->hrec.assign((size_t)count, BRec{});
    const int st = batch_alloc(b);
    if (st != LP_PIVOTED) {
        g_batch_err = b->err;
        lp_batch_destroy(b);
        return st;
    }
    *out = b;
    return LP_PIVOTED;
}

extern "C" int lp_placed_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, int place,
                                lp_batch **out)
{
    return create_uniform(count, m, n, log_cap, device, place, 1, out);
}

extern "C" int lp_teamed_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device, int place,
                                int team, lp_batch **out)
{
    return create_uniform(count, m, n, log_cap, device, place, team, out);
}

extern "C" int lp_batch_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device,
                               lp_batch **out)
{
    return lp_placed_create(count, m, n, log_cap, device, LP_PLACE_LDS, out);
}

extern "C" int lp_ragged_create(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device,
                                lp_batch **out)
{
    return lp_placed_create_ragged(count, m, n, log_cap, device, LP_PLACE_LDS, out);
}

static int create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device, int place,
                         const int32_t *team, lp_batch **out);

extern "C" int lp_placed_create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap,
                                       int device, int place, lp_batch **out)
{
    return create_ragged(count, m, n, log_cap, device, place, nullptr, out);
}

extern "C" int lp_teamed_create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap,
                                       int device, int place, const int32_t *team, lp_batch **out)
{
    return create_ragged(count, m, n, log_cap, device, place, team, out);
}

// lp_placed_create_ragged with one team request per LP (null: 1 for every LP)
static int create_ragged(int64_t count, const int64_t *m, const int64_t *n, int64_t log_cap, int device, int place,
                         const int32_t *team, lp_batch **out)
{
    if (!out) {
        g_batch_err = "out is NULL";
        return LP_BAD_ARG;
    }
    *out = nullptr;
    if (place != LP_PLACE_LDS && place != LP_PLACE_AUTO && place != LP_PLACE_DEVICE) {
        g_batch_err = "unknown place: LP_PLACE_LDS, LP_PLACE_AUTO or LP_PLACE_DEVICE";
        return LP_BAD_ARG;
    }
    if (count <= 0 || !m || !n || log_cap < 0) {
        g_batch_err = "need count > 0, shape arrays m and n, and log_cap >= 0";
        return LP_BAD_ARG;
    }
    if (count > INT_MAX || log_cap > (INT64_MAX >> 5) / count) {
        g_batch_err = "batch too large: count or count x log_cap out of range";
        return LP_BAD_ARG;
    }
    for (int64_t i = 0; i < count; ++i)
        if (m[i] <= 0 || n[i] <= 0) {
            g_batch_err = "LP " + std::to_string(i) + ": need m > 0 and n > 0";
            return LP_BAD_ARG;
        }
    std::vector<uint8_t> on_device((size_t)count, 0);
    bool any = false;
    for (int64_t i = 0; i < count; ++i) {
        const int req = team ? team[i] : 1;
        if (req != 1) {
            if (req > 1 && place == LP_PLACE_LDS) {
                g_batch_err = "LP " + std::to_string(i) + ": " + TEAM_NEEDS_DEVICE;
                return LP_BAD_ARG;
            }
            const std::string why = m[i] < (1 << 20) && n[i] < (1 << 20) ? team_refusal(req, m[i], n[i]) : "";
            if (!why.empty()) {
                g_batch_err = "LP " + std::to_string(i) + ": " + why;
                return LP_BAD_ARG;
            }
        }
        // a teamed LP is always device-placed
        const int where = lpk::plan_place(req > 1 ? (int)LP_PLACE_DEVICE : place, m[i], n[i]);
        if (where == lpk::PLAN_PLACE_TOO_LARGE && place == LP_PLACE_LDS) {
            g_batch_err = "LP " + std::to_string(i) + " (" + std::to_string(m[i]) + " x " + std::to_string(n[i]) +
                          ") is too large for the batch path: (m+1) x (n+1) float64 plus its side buffers must "
                          "fit one CU's 160 KiB of LDS (use lp_create)";
            return LP_BAD_ARG;
        }
        if (where < 0) {
            g_batch_err = "LP " + std::to_string(i) + " (" + std::to_string(m[i]) + " x " + std::to_string(n[i]) +
                          ") is " + DEV_TOO_LARGE;
            return LP_BAD_ARG;
        }
        on_device[(size_t)i] = where == lpk::PLAN_PLACE_DEVICE;
        any = any || where == lpk::PLAN_PLACE_DEVICE;
    }
    lp_batch *b = new lp_batch;
    b->dev = device;
    b->count = count;
    b->logcap = log_cap;
    b->ragged = true;
    b->place = place;
    b->lp_on_device = std::move(on_device);
    b->any_on_device = any;
    if (team) b->team_req.assign(team, team + count);
    b->hshape.resize((size_t)count);
    lpk::BShape at{};       // the running offsets
    for (int64_t i = 0; i < count; ++i) {
        lpk::BShape &s = b->hshape[(size_t)i];
        s = at;
        s.m = (int32_t)m[i];
        s.n = (int32_t)n[i];
        s.pitch = (int32_t)lpk::plan_plain_pitch(n[i]);
        s.wpitch = (int32_t)lpk::plan_twophase_pitch(m[i], n[i]);
        at.toff += (m[i] + 1) * (n[i] + 1);
        at.boff += m[i];
        at.woff += (m[i] + 1) * (n[i] + 1 + m[i]);
        at.coff += n[i];
    }
    lp_default_tol(&b->tol);
    b->hrec.assign((size_t)count, BRec{});
    const int st = batch_alloc(b);
    if (st != LP_PIVOTED) {
        g_batch_err = b->err;
        lp_batch_destroy(b);
        return st;
    }
    *out = b;
    return LP_PIVOTED;
}

extern "C" int lp_ragged_shape(const lp_batch *b, int64_t index, int64_t *m, int64_t *n)
{
    if (!b) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    if (m) *m = b->lp_m(index);
    if (n) *n = b->lp_n(index);
    return LP_PIVOTED;
}

// the bins of plan tp in lp_ragged_plan's format
static int plan_report(lp_batch *b, int tp, int64_t *bins, int64_t cap, int64_t *count)
{
    if (!b) return LP_BAD_ARG;
    if (cap < 0 || (cap > 0 && !bins)) return bfail(b, "bad bins buffer");
    const int st = ensure_plan(b, tp);
    if (st != LP_PIVOTED) return st;
    const std::vector<lpk::PlanBin> &B = b->plan[tp].bins;
    if (count) *count = (int64_t)B.size();
    for (size_t k = 0; k < B.size() && (int64_t)k < cap; ++k) {
        bins[4 * k] = B[k].waves;
        bins[4 * k + 1] = B[k].lds;
        bins[4 * k + 2] = (int64_t)B[k].order.size();
        bins[4 * k + 3] = B[k].lps_per_cu;
    }
    return LP_PIVOTED;
}

extern "C" int lp_ragged_plan(lp_batch *b, int twophase, int64_t *bins, int64_t cap, int64_t *count)
{
    return plan_report(b, twophase ? 1 : 0, bins, cap, count);
}

extern "C" int lp_phased_plan(lp_batch *b, int64_t *bins, int64_t cap, int64_t *count)
{
    return plan_report(b, 2, bins, cap, count);
}

extern "C" int64_t lp_phased_lds_bytes(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0) return LP_BAD_ARG;
    return lpk::plan_phased_lds(m, n);
}

extern "C" int lp_phased_placement(const lp_batch *b, int64_t index, int *place)
{
    if (!b || !place) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    const int where = lpk::plan_place_phased(b->place, b->lp_m(index), b->lp_n(index));
    if (where < 0) return LP_BAD_ARG;       // too large for either placement: lp_phased_solve names it
    *place = where;
    return LP_PIVOTED;
}

extern "C" const char *lp_batch_last_error(const lp_batch *b)
{
    return b ? b->err.c_str() : g_batch_err.c_str();
}

extern "C" int lp_batch_set_tol(lp_batch *b, const lp_tol *tol)
{
    if (!b) return LP_BAD_ARG;
    if (!tol) return bfail(b, "tol is NULL");
    b->tol = *tol;
    return LP_PIVOTED;
}

extern "C" int lp_batch_set_chunk(lp_batch *b, int64_t pivots_per_launch)
{
    if (!b) return LP_BAD_ARG;
    if (pivots_per_launch < 1) return bfail(b, "pivots_per_launch must be >= 1");
    b->chunk = pivots_per_launch;
    return LP_PIVOTED;
}

static int window_ok(lp_batch *b, int64_t first, int64_t count, const void *p, int64_t ldh)
{
    if (first < 0 || count < 0 || first > b->count || count > b->count - first)
        return bfail(b, "LP range out of bounds");
    if (count > 0 && !p) return bfail(b, "host buffer is NULL");
    if (!b->ragged && ldh < b->n + 1) return bfail(b, "ldh < n + 1");
    return LP_PIVOTED;
}

static void window_reset(lp_batch *b, int64_t first, int64_t count)
{
    for (int64_t i = first; i < first + count; ++i) {
        b->hrec[(size_t)i] = BRec{};
        if (!b->nlog.empty()) b->nlog[(size_t)i] = 0;
        if (!b->short_rows.empty()) b->short_rows[(size_t)i] = 0;
    }
}

// The packed layout: LP after LP, each (m_i+1) x (n_i+1) row-major without
// padding -- how both kinds of batch keep their tableaux on the device, so a
// window is one contiguous copy.
extern "C" int lp_ragged_upload(lp_batch *b, int64_t first, int64_t count, const double *src)
{
    if (!b) return LP_BAD_ARG;
    const int st = window_ok(b, first, count, src, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    const int64_t at = b->toff(first), elems = b->toff(first + count) - at;
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpyAsync(b->T + at, src, (size_t)elems * sizeof(double), hipMemcpyHostToDevice, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    window_reset(b, first, count);
    return LP_PIVOTED;
}

extern "C" int lp_ragged_download(lp_batch *b, int64_t first, int64_t count, double *dst)
{
    if (!b) return LP_BAD_ARG;
    const int st = window_ok(b, first, count, dst, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    const int64_t at = b->toff(first), elems = b->toff(first + count) - at;
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpyAsync(dst, b->T + at, (size_t)elems * sizeof(double), hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

extern "C" int lp_batch_upload(lp_batch *b, int64_t first, int64_t count, const double *src,
                               int64_t ldh)
{
    if (!b) return LP_BAD_ARG;
    if (b->ragged) return bfail(b, "a ragged batch has no common ldh: use lp_ragged_upload");
    const int st = window_ok(b, first, count, src, ldh);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    const size_t w = (size_t)(b->n + 1) * sizeof(double), rows = (size_t)(b->m + 1);
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpy2DAsync(b->T + (size_t)first * rows * (size_t)(b->n + 1), w, src,
                             (size_t)ldh * sizeof(double), w, (size_t)count * rows,
                             hipMemcpyHostToDevice, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    window_reset(b, first, count);
    return LP_PIVOTED;
}

extern "C" int lp_batch_download(lp_batch *b, int64_t first, int64_t count, double *dst, int64_t ldh)
{
    if (!b) return LP_BAD_ARG;
    if (b->ragged) return bfail(b, "a ragged batch has no common ldh: use lp_ragged_download");
    const int st = window_ok(b, first, count, dst, ldh);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    const size_t w = (size_t)(b->n + 1) * sizeof(double), rows = (size_t)(b->m + 1);
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpy2DAsync(dst, (size_t)ldh * sizeof(double),
                             b->T + (size_t)first * rows * (size_t)(b->n + 1), w, w,
                             (size_t)count * rows, hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// packed: LP i's m_i entries after those of the LPs before it (count x m on a
// uniform batch)
extern "C" int lp_ragged_set_basis(lp_batch *b, const int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (!basis) {
        b->basis_on = false;
        return LP_PIVOTED;
    }
    const size_t bytes = (size_t)b->boff(b->count) * sizeof(int32_t);
    BCHK(b, hipSetDevice(b->dev));
    if (!b->basis) BCHK(b, hipMalloc(&b->basis, bytes));
    BCHK(b, hipMemcpyAsync(b->basis, basis, bytes, hipMemcpyHostToDevice, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    b->basis_on = true;
    return LP_PIVOTED;
}

extern "C" int lp_batch_set_basis(lp_batch *b, const int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (b->ragged) return bfail(b, "a ragged batch has no count x m basis: use lp_ragged_set_basis");
    return lp_ragged_set_basis(b, basis);
}

extern "C" int lp_ragged_get_basis(lp_batch *b, int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (!basis) return bfail(b, "basis is NULL");
    if (!b->basis_on) return bfail(b, "no basis attached (lp_batch_set_basis)");
    const size_t bytes = (size_t)b->boff(b->count) * sizeof(int32_t);
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpyAsync(basis, b->basis, bytes, hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

extern "C" int lp_batch_get_basis(lp_batch *b, int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (b->ragged) return bfail(b, "a ragged batch has no count x m basis: use lp_ragged_get_basis");
    return lp_ragged_get_basis(b, basis);
}

// what a uniform batch's one grid runs with (a ragged batch takes these from its plan's bins)
struct UniformLaunch {
    size_t lds;
    bool device;
    int waves;
};

// One launch for every unfinished LP of a call, on the batch's stream.  FULL is the device-placed
// form's args (DArgs or PArgs: the call's args, the bin and `work`); an LDS-placed launch reads its
// base, FULL::Lds.  A uniform batch is one grid.  A ragged batch is one launch per bin of plan
// `tp`, largest LDS first and the device-placed LPs before those; a bin whose LPs are all finished
// is not launched again.
template <template <bool> class FULL, bool RAGGED, class CORE>
static int launch_unfinished(lp_batch *b, int tp, KFamily lds_family, KFamily dev_family, bool maxinc, bool dual,
                             const CORE &A, const UniformLaunch &U)
{
    FULL<RAGGED> F{};
    static_cast<CORE &>(F) = A;
    F.work = BATCH_DEV_WORK;
    void *const full = &F, *const lds = static_cast<typename FULL<RAGGED>::Lds *>(&F);
    if constexpr (RAGGED) {
        F.R = {b->shape, b->order[tp], 0};
        for (const lpk::PlanBin &bin : b->plan[tp].bins) {
            F.R.nbin = (int)bin.order.size();
            if (bin_unfinished(b, bin)) {
                launch({bin.device ? dev_family : lds_family, true, bin.waves, maxinc, dual}, dim3((unsigned)F.R.nbin),
                       (size_t)bin.lds, b->s, bin.device ? full : lds);
                BCHK(b, hipGetLastError());
            }
            F.R.order += F.R.nbin;
        }
    } else {
        launch({U.device ? dev_family : lds_family, false, U.waves, maxinc, dual}, dim3((unsigned)b->count), U.lds,
               b->s, U.device ? full : lds);
        BCHK(b, hipGetLastError());
    }
    return LP_PIVOTED;
}

// The relaunch loop of every call: enqueue() launches for the unfinished LPs, the records come
// back, and the loop ends when no LP is left.  teamed (the plain call of a batch with teams): a
// teamed LP's record is the one its last launch wrote, which enqueue() has copied to hrec_team.
template <class Enqueue>
static int drive(lp_batch *b, bool teamed, Enqueue enqueue)
{
    const size_t rbytes = (size_t)b->count * sizeof(BRec);
    for (;;) {
        const int st = enqueue();
        if (st != LP_PIVOTED) return st;
        BCHK(b, hipMemcpyAsync(b->hrec.data(), b->rec, rbytes, hipMemcpyDeviceToHost, b->s));
        BCHK(b, hipStreamSynchronize(b->s));
        if (teamed)
            for (const lpk::TeamWG &w : b->hwg)
                if (w.rank == 0) b->hrec[(size_t)w.lp] = b->hrec_team[(size_t)w.lp];
        bool more = false;
        for (const BRec &r : b->hrec)
            if (r.state != lpk::B_DONE) {
                more = true;
                break;
            }
        if (!more) return LP_PIVOTED;
    }
}

// One lpf_solve / lpf_run per LP: bounded launches until every record is done.
static int batch_drive(lp_batch *b, int mode, int rule, int64_t limit)
{
    BCHK(b, hipSetDevice(b->dev));
    const size_t rbytes = (size_t)b->count * sizeof(BRec);
    b->hrec.assign((size_t)b->count, BRec{});        // B_START
    b->nlog.clear();
    BCHK(b, hipMemcpyAsync(b->rec, b->hrec.data(), rbytes, hipMemcpyHostToDevice, b->s));
    BArgs A{};
    A.T = b->T;
    A.rec = b->rec;
    A.log = b->log;
    A.basis = b->basis_on ? b->basis : nullptr;
    A.count = b->count;
    A.logcap = b->log ? b->logcap : 0;
    A.chunk = b->chunk;
    A.limit = limit;
    A.m = (int)b->m;
    A.n = (int)b->n;
    A.pitch = b->pitch;
    A.mode = mode;
    A.run_rule = rule;
    A.tol = b->tol;
    // LP_RULE_MAX_INCREASE: the instantiations that carry its column scan
    const bool maxinc = mode == lpk::MODE_RUN && rule == LP_RULE_MAX_INCREASE;
    // LP_RULE_DUAL: likewise
    const bool dual = mode == lpk::MODE_RUN && rule == LP_RULE_DUAL;
    // teamed LPs: a round trip enqueues `window` launches of
    // k_batch_team, one pivot each, the record arrays taking turns, and reads
    // the last one written back once
    const bool teamed = !b->hwg.empty();
    BRec *const recs[2] = {b->rec, b->rec2};
    int rin = 0;                    // the array the next teamed launch reads: B_START is in b->rec
    if (teamed) b->hrec_team.assign((size_t)b->count, BRec{});
    // one launch over the workgroup table (K_TEAM or K_TEAM_HOME): reads recs[rin], writes the other array
    auto team_args = [&](auto MA, KFamily family, size_t lds) {
        static_cast<BArgs &>(MA) = A;
        MA.T2 = b->T2;
        MA.rec_in = recs[rin];
        MA.rec_out = recs[rin ^ 1];
        MA.wg = b->wg;
        MA.nwg = (int)b->hwg.size();
        if constexpr (std::is_same_v<decltype(MA), lpk::MArgs<true>>) MA.R = {b->shape, nullptr, 0};
        launch({family, b->ragged}, dim3((unsigned)b->hwg.size()), lds, b->s, &MA);
    };
    auto team_pass = [&](KFamily family, size_t lds) {
        if (b->ragged) team_args(lpk::MArgs<true>{}, family, lds);
        else team_args(lpk::MArgs<false>{}, family, lds);
    };
    auto team_unfinished = [&]() {
        for (const lpk::TeamWG &w : b->hwg)
            if (b->hrec[(size_t)w.lp].state != lpk::B_DONE) return true;
        return false;
    };
    const UniformLaunch U{b->lds, b->on_device, b->waves};
    const int st = drive(b, teamed, [&]() -> int {
        if (teamed && team_unfinished()) {      // first: they run longest
            for (int64_t k = 0; k < b->window; ++k, rin ^= 1) {
                team_pass(K_TEAM, b->team_lds);
                BCHK(b, hipGetLastError());
            }
            BCHK(b, hipMemcpyAsync(b->hrec_team.data(), recs[rin], rbytes, hipMemcpyDeviceToHost, b->s));
        }
        if (b->ragged) return launch_unfinished<lpk::DArgs, true>(b, 0, K_PLAIN, K_DEVICE, maxinc, dual, A, U);
        if (teamed) return LP_PIVOTED;          // a uniform batch: every LP has the one team
        return launch_unfinished<lpk::DArgs, false>(b, 0, K_PLAIN, K_DEVICE, maxinc, dual, A, U);
    });
    if (st != LP_PIVOTED || !teamed) return st;
    // an LP that ends in its second buffer goes home to b->T: one launch
    bool away = false;
    for (const lpk::TeamWG &w : b->hwg) away = away || b->hrec[(size_t)w.lp].buf != 0;
    if (!away) return LP_PIVOTED;
    // (recs[rin]: the array the last launch wrote)
    team_pass(K_TEAM_HOME, 0);
    BCHK(b, hipGetLastError());
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

extern "C" int lp_batch_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int64_t *npiv,
                              int64_t *nstd)
{
    if (!b) return LP_BAD_ARG;
    const int st = batch_drive(b, lpk::MODE_SOLVE, LP_RULE_STANDARD, max_pivots < 0 ? -1 : max_pivots);
    if (st != LP_PIVOTED) return st;
    for (int64_t i = 0; i < b->count; ++i) {
        const BRec &r = b->hrec[(size_t)i];
        if (status) status[i] = r.status;
        if (npiv) npiv[i] = r.npiv;
        if (nstd) nstd[i] = r.nstd;
    }
    return 0;
}

extern "C" int lp_batch_run(lp_batch *b, int rule, int64_t k, int32_t *status, int64_t *done)
{
    if (!b) return LP_BAD_ARG;
    if (rule != LP_RULE_STANDARD && rule != LP_RULE_MIN_INDEX && rule != LP_RULE_MAX_INCREASE && rule != LP_RULE_DUAL)
        return bfail(b, "unknown rule");
    if (k < 0) return bfail(b, "k < 0");
    if (rule == LP_RULE_DUAL && !b->hwg.empty())
        return bfail(b, "LP_RULE_DUAL is not available on a batch that has a team above 1: every workgroup of a team "
                        "would scan column 0 and two rows alike (use a batch without teams)");
    if (rule == LP_RULE_MAX_INCREASE && !b->hwg.empty())
        return bfail(b, "LP_RULE_MAX_INCREASE is not available on a batch that has a team above 1: every workgroup "
                        "of a team would scan the whole tableau (use a batch without teams, or rule 0 or 1)");
    const int st = batch_drive(b, lpk::MODE_RUN, rule, k);
    if (st != LP_PIVOTED) return st;
    for (int64_t i = 0; i < b->count; ++i) {
        const BRec &r = b->hrec[(size_t)i];
        if (status) status[i] = r.status;
        if (done) done[i] = r.npiv;
    }
    return 0;
}

extern "C" int lp_batch_objective(lp_batch *b, double *z)
{
    if (!b) return LP_BAD_ARG;
    if (!z) return bfail(b, "z is NULL");
    BCHK(b, hipSetDevice(b->dev));
    if (b->ragged) {        // no common stride: gather T[toff[i]] on the device
        if (!b->zbuf) BCHK(b, hipMalloc(&b->zbuf, (size_t)b->count * sizeof(double)));
        hipLaunchKernelGGL(lpk::k_gather_z, dim3((unsigned)((b->count + 255) / 256)), dim3(256), 0, b->s, b->T,
                           b->shape, b->zbuf, (long long)b->count);
        BCHK(b, hipGetLastError());
        BCHK(b, hipMemcpyAsync(z, b->zbuf, (size_t)b->count * sizeof(double), hipMemcpyDeviceToHost, b->s));
    } else {
        const size_t lp_bytes = (size_t)(b->m + 1) * (size_t)(b->n + 1) * sizeof(double);
        BCHK(b, hipMemcpy2DAsync(z, sizeof(double), b->T, lp_bytes, sizeof(double), (size_t)b->count,
                                 hipMemcpyDeviceToHost, b->s));
    }
    BCHK(b, hipStreamSynchronize(b->s));
    for (int64_t i = 0; i < b->count; ++i) z[i] = -z[i];
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// batch solutions on the device
// ---------------------------------------------------------------------------

static int solution_window(lp_batch *b, int64_t first, int64_t count)
{
    if (first < 0 || count < 0 || first > b->count || count > b->count - first)
        return bfail(b, "LP range out of bounds");
    return LP_PIVOTED;
}

// what both calls launch with: the window, its tableau columns and basis entries
static lpk::SArgs solution_args(const lp_batch *b, int64_t first, int64_t count)
{
    lpk::SArgs A{};
    A.T = b->T;
    A.basis = b->basis;
    A.shape = b->ragged ? b->shape : nullptr;
    A.first = first;
    A.count = count;
    A.lanes = b->coff(first + count) - b->coff(first) + count;
    A.nbasis = b->boff(first + count) - b->boff(first);
    A.m = (int)b->m;
    A.n = (int)b->n;
    return A;
}

#define SLAUNCH(b, kern, grid, A)                                                                          \
    do {                                                                                                   \
        if ((b)->ragged)                                                                                   \
            hipLaunchKernelGGL(lpk::kern<true>, dim3((unsigned)(grid).blocks), dim3((grid).threads), 0, (b)->s, A); \
        else                                                                                               \
            hipLaunchKernelGGL(lpk::kern<false>, dim3((unsigned)(grid).blocks), dim3((grid).threads), 0, (b)->s, A); \
        BCHK(b, hipGetLastError());                                                                        \
    } while (0)

extern "C" int lp_solution_canonical(lp_batch *b, int64_t first, int64_t count, int32_t *flags, int64_t *first_bad)
{
    if (!b) return LP_BAD_ARG;
    const int st = solution_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (count == 0) {
        if (first_bad) *first_bad = -1;
        return LP_PIVOTED;
    }
    lpk::SArgs A = solution_args(b, first, count);
    int64_t max_m = b->m;
    if (b->ragged) {
        max_m = 0;
        for (int64_t i = first; i < first + count; ++i) max_m = std::max(max_m, b->lp_m(i));
    }
    const lpk::FlatGrid scan = lpk::plan_scan_grid(A.lanes, max_m);
    const lpk::FlatGrid init =
        lpk::plan_flat_grid(std::max<int64_t>(A.nbasis, count), lpk::PLAN_FLAT_THREADS, lpk::PLAN_FLAT_THREADS);
    const lpk::FlatGrid fin = lpk::plan_flat_grid(A.nbasis, lpk::PLAN_FLAT_THREADS, lpk::PLAN_FLAT_THREADS);
    if (scan.blocks < 0 || init.blocks < 0) return bfail(b, "window too large for one launch: derive it in parts");
    BCHK(b, hipSetDevice(b->dev));
    const size_t bbytes = (size_t)b->boff(b->count) * sizeof(int32_t);
    if (!b->basis) BCHK(b, hipMalloc(&b->basis, bbytes));
    if (!b->canon) BCHK(b, hipMalloc(&b->canon, sizeof(unsigned long long) + (size_t)b->count * sizeof(int32_t)));
    if (!b->basis_on) BCHK(b, hipMemsetAsync(b->basis, 0xFF, bbytes, b->s));     // -1 outside the window
    A.basis = b->basis;
    A.bad = b->canon;
    A.flags = reinterpret_cast<int32_t *>(b->canon + 1);
    SLAUNCH(b, k_canon_init, init, A);
    SLAUNCH(b, k_canon_scan, scan, A);
    SLAUNCH(b, k_canon_finish, fin, A);
    unsigned long long bad = ~0ull;
    BCHK(b, hipMemcpyAsync(&bad, A.bad, sizeof bad, hipMemcpyDeviceToHost, b->s));
    if (flags)
        BCHK(b, hipMemcpyAsync(flags, A.flags, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    b->basis_on = true;
    if (first_bad) *first_bad = bad == ~0ull ? -1 : (int64_t)bad;
    return LP_PIVOTED;
}

extern "C" int lp_solution_gather(lp_batch *b, int64_t first, int64_t count, double *x, double *z)
{
    if (!b) return LP_BAD_ARG;
    const int st = solution_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (!b->basis_on) return bfail(b, "no basis attached (lp_batch_set_basis)");
    if (count == 0) return LP_PIVOTED;
    lpk::SArgs A = solution_args(b, first, count);
    const lpk::FlatGrid grid = lpk::plan_flat_grid(A.lanes, lpk::PLAN_FLAT_THREADS, lpk::PLAN_FLAT_THREADS);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: gather it in parts");
    BCHK(b, hipSetDevice(b->dev));
    const int64_t xall = b->coff(b->count);
    if (!b->sol) BCHK(b, hipMalloc(&b->sol, (size_t)(xall + b->count) * sizeof(double)));
    A.x = b->sol;
    A.z = b->sol + xall;
    SLAUNCH(b, k_solution, grid, A);
    if (x)
        BCHK(b, hipMemcpyAsync(x, A.x, (size_t)(A.lanes - count) * sizeof(double), hipMemcpyDeviceToHost, b->s));
    if (z) BCHK(b, hipMemcpyAsync(z, A.z, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// problem-form batches
// ---------------------------------------------------------------------------

static_assert(lpk::PLAN_SENSE_LE == LP_SENSE_LE && lpk::PLAN_SENSE_GE == LP_SENSE_GE &&
                  lpk::PLAN_SENSE_EQ == LP_SENSE_EQ,
              "batch_plan.h mirrors LP_SENSE_*");

extern "C" int64_t lp_problem_columns(const int8_t *sense, int64_t m, int64_t ns)
{
    if (!sense || m <= 0 || ns <= 0) return LP_BAD_ARG;
    int64_t k = 0;
    for (int64_t r = 0; r < m; ++r) {
        if (sense[r] < LP_SENSE_LE || sense[r] > LP_SENSE_EQ) return LP_BAD_ARG;
        k += sense[r] != LP_SENSE_EQ ? 1 : 0;
    }
    return ns + k;
}

extern "C" int lp_problem_set_senses(lp_batch *b, const int8_t *sense)
{
    if (!b) return LP_BAD_ARG;
    if (!sense) {
        b->senses_on = false;
        return LP_PIVOTED;
    }
    // everything is derived on the host first: a refusal changes nothing
    const int64_t nl = b->ragged ? b->count : 1;
    std::vector<int32_t> tab((size_t)(b->ragged ? b->boff(b->count) : b->m));
    std::vector<lpk::PInfo> info((size_t)b->count + 1);
    int64_t poff = 0;
    for (int64_t i = 0; i < nl; ++i) {
        const int64_t m = b->lp_m(i), n = b->lp_n(i), at = b->ragged ? b->boff(i) : 0;
        int64_t row = -1;
        const int64_t ns = lpk::plan_problem_slack(sense + at, m, n, tab.data() + at, &row);
        if (ns == lpk::PLAN_PROBLEM_BAD_SENSE) {
            b->err = (b->ragged ? "LP " + std::to_string(i) + ", row " : std::string("every LP, row ")) +
                     std::to_string(row) + ": sense " + std::to_string((int)sense[at + row]) +
                     " is not LP_SENSE_LE (0), LP_SENSE_GE (1) or LP_SENSE_EQ (2)";
            return LP_BAD_ARG;
        }
        if (ns < 0) {
            int64_t k = 0;
            for (int64_t r = 0; r < m; ++r) k += sense[at + r] != LP_SENSE_EQ ? 1 : 0;
            b->err = (b->ragged ? "LP " + std::to_string(i) : std::string("every LP")) + ": its k = " +
                     std::to_string(k) + " slack columns leave no structural variable among n = " + std::to_string(n);
            return LP_BAD_ARG;
        }
        info[(size_t)i] = lpk::PInfo{poff, (int32_t)ns, 0};
        poff += (m + 1) * (ns + 1);
    }
    if (!b->ragged)
        for (int64_t i = 1; i < b->count; ++i) info[(size_t)i] = lpk::PInfo{i * poff, info[0].ns, 0};
    info[(size_t)b->count] = lpk::PInfo{b->ragged ? poff : b->count * poff, 0, 0};
    BCHK(b, hipSetDevice(b->dev));
    if (!b->slack) BCHK(b, hipMalloc(&b->slack, tab.size() * sizeof(int32_t)));
    if (b->ragged && !b->pinfo) BCHK(b, hipMalloc(&b->pinfo, (size_t)b->count * sizeof(lpk::PInfo)));
    b->senses_on = false;       // until both copies have landed
    BCHK(b, hipMemcpyAsync(b->slack, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, b->s));
    if (b->ragged)
        BCHK(b, hipMemcpyAsync(b->pinfo, info.data(), (size_t)b->count * sizeof(lpk::PInfo), hipMemcpyHostToDevice,
                               b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    b->hinfo = std::move(info);
    b->hslack = std::move(tab);
    b->senses_on = true;
    return LP_PIVOTED;
}

extern "C" int lp_problem_vars(const lp_batch *b, int64_t index, int64_t *ns)
{
    if (!b || !ns || !b->senses_on) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    *ns = b->hinfo[(size_t)index].ns;
    return LP_PIVOTED;
}

// the window as k_assemble and k_duals take it
static lpk::FArgs problem_args(const lp_batch *b, int64_t first, int64_t count)
{
    lpk::FArgs A{};
    A.S = solution_args(b, first, count);
    A.out = b->T;
    A.slack = b->slack;
    A.info = b->ragged ? b->pinfo : nullptr;
    A.elems = b->toff(first + count) - b->toff(first);
    A.ns = b->hinfo.empty() ? 0 : b->hinfo[0].ns;
    return A;
}

extern "C" int lp_problem_upload(lp_batch *b, int64_t first, int64_t count, const double *src)
{
    if (!b) return LP_BAD_ARG;
    if (!b->senses_on) return bfail(b, "no senses attached (lp_problem_set_senses)");
    const int st = window_ok(b, first, count, src, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    lpk::FArgs A = problem_args(b, first, count);
    const lpk::FlatGrid grid = lpk::plan_assemble_grid(A.elems);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: upload it in parts");
    const int64_t at = b->hinfo[(size_t)first].poff, elems = b->hinfo[(size_t)(first + count)].poff - at;
    BCHK(b, hipSetDevice(b->dev));
    const int64_t all = b->hinfo[(size_t)b->count].poff;
    if (b->pstage_cap < all) {      // the first call, or senses with fewer equalities since
        if (b->pstage) BCHK(b, hipFree(b->pstage));
        b->pstage = nullptr;
        b->pstage_cap = 0;
        BCHK(b, hipMalloc(&b->pstage, (size_t)all * sizeof(double)));
        b->pstage_cap = all;
    }
    BCHK(b, hipMemcpyAsync(b->pstage, src, (size_t)elems * sizeof(double), hipMemcpyHostToDevice, b->s));
    A.src = b->pstage;
    SLAUNCH(b, k_assemble, grid, A);
    BCHK(b, hipStreamSynchronize(b->s));
    window_reset(b, first, count);
    return LP_PIVOTED;
}

extern "C" int lp_problem_duals(lp_batch *b, int64_t first, int64_t count, double *y)
{
    if (!b) return LP_BAD_ARG;
    if (!b->senses_on) return bfail(b, "no senses attached (lp_problem_set_senses)");
    const int st = window_ok(b, first, count, y, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    lpk::FArgs A = problem_args(b, first, count);
    const lpk::FlatGrid grid = lpk::plan_flat_grid(A.S.nbasis, lpk::PLAN_FLAT_THREADS, lpk::PLAN_FLAT_THREADS);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: read the duals in parts");
    BCHK(b, hipSetDevice(b->dev));
    if (!b->dual) BCHK(b, hipMalloc(&b->dual, (size_t)b->boff(b->count) * sizeof(double)));
    A.S.x = b->dual;
    SLAUNCH(b, k_duals, grid, A);
    BCHK(b, hipMemcpyAsync(y, b->dual, (size_t)A.S.nbasis * sizeof(double), hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// warm re-solves
// ---------------------------------------------------------------------------

// an LP whose last two-phase call left fewer than m live rows: the message, and true
static bool short_rows_refused(lp_batch *b, int64_t i)
{
    if (b->short_rows.empty() || !b->short_rows[(size_t)i]) return false;
    const int64_t live = b->htrec[(size_t)i].rows;
    b->err = "LP " + std::to_string(i) + ", row " + std::to_string(live) + ": its last two-phase call left " +
             std::to_string(live) + " of " + std::to_string(b->lp_m(i)) + " rows live";
    return true;
}

extern "C" int lp_resolve_set_rhs(lp_batch *b, int64_t first, int64_t count, const double *rhs)
{
    if (!b) return LP_BAD_ARG;
    if (!b->senses_on) return bfail(b, "no senses attached (lp_problem_set_senses)");
    const int st = window_ok(b, first, count, rhs, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    // everything is checked on the host first: a refusal copies and launches nothing
    for (int64_t i = first; i < first + count; ++i) {
        const int64_t m = b->lp_m(i), at = b->ragged ? b->boff(i) : 0;
        for (int64_t r = 0; r < m; ++r)
            if (b->hslack[(size_t)(at + r)] == 0) {
                b->err = "LP " + std::to_string(i) + ", row " + std::to_string(r) +
                         " is an equality: it owns no column that holds the basis inverse, as for its dual";
                return LP_BAD_ARG;
            }
        if (short_rows_refused(b, i)) return LP_BAD_ARG;
    }
    lpk::FArgs A = problem_args(b, first, count);
    A.S.lanes = A.S.nbasis + count;
    const lpk::FlatGrid grid = lpk::plan_rhs_grid(A.S.lanes);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: set it in parts");
    BCHK(b, hipSetDevice(b->dev));
    if (!b->rhs) BCHK(b, hipMalloc(&b->rhs, (size_t)(b->boff(b->count) + b->count) * sizeof(double)));
    BCHK(b, hipMemcpyAsync(b->rhs, rhs, (size_t)A.S.lanes * sizeof(double), hipMemcpyHostToDevice, b->s));
    A.S.x = b->rhs;
    SLAUNCH(b, k_rhs, grid, A);
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// general-form batches
// ---------------------------------------------------------------------------

static_assert(lpk::PLAN_VAR_PLAIN == LP_VAR_PLAIN && lpk::PLAN_VAR_LOWER == LP_VAR_LOWER &&
                  lpk::PLAN_VAR_BOXED == LP_VAR_BOXED && lpk::PLAN_VAR_UPPER == LP_VAR_UPPER &&
                  lpk::PLAN_VAR_FREE == LP_VAR_FREE,
              "batch_plan.h mirrors LP_VAR_*");

extern "C" int64_t lp_general_rows(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns)
{
    lpk::GeneralCounts c;
    return lpk::plan_general_counts(sense, kind, m, ns, &c) == 0 ? c.rows : (int64_t)LP_BAD_ARG;
}

extern "C" int64_t lp_general_columns(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns)
{
    lpk::GeneralCounts c;
    return lpk::plan_general_counts(sense, kind, m, ns, &c) == 0 ? c.cols : (int64_t)LP_BAD_ARG;
}

extern "C" int lp_general_set_form(lp_batch *b, const int64_t *m, const int64_t *ns, const int8_t *sense,
                                   const int8_t *kind, const int8_t *maximise)
{
    if (!b) return LP_BAD_ARG;
    if (!sense) {
        b->form_on = false;
        return LP_PIVOTED;
    }
    if (!m || !ns || !kind || !maximise) return bfail(b, "m, ns, kind or maximise is NULL");
    // everything is derived on the host first: a refusal changes nothing
    const int64_t nl = b->ragged ? b->count : 1;
    const std::string every = "every LP";
    std::vector<lpk::GInfo> info((size_t)b->count + 1);
    std::vector<lpk::GVar> var;
    std::vector<int32_t> slack((size_t)(b->ragged ? b->boff(b->count) : b->m)), bvar(slack.size());
    int64_t poff = 0, voff = 0, yoff = 0, sat = 0;
    for (int64_t i = 0; i < nl; ++i) {
        const std::string who = b->ragged ? "LP " + std::to_string(i) : every;
        lpk::GeneralCounts c;
        int64_t bad = -1;
        // m' >= m and n' > ns: a larger m or ns cannot fit, and its entries are not read
        const bool fits = m[i] >= 1 && ns[i] >= 1 && m[i] <= b->lp_m(i) && ns[i] <= b->lp_n(i);
        const int64_t st = !fits ? lpk::PLAN_GENERAL_BAD_SHAPE
                                 : lpk::plan_general_counts(sense + yoff, kind + voff, m[i], ns[i], &c, &bad);
        if (st == lpk::PLAN_GENERAL_BAD_SENSE) {
            b->err = who + ", row " + std::to_string(bad) + ": sense " + std::to_string((int)sense[yoff + bad]) +
                     " is not LP_SENSE_LE (0), LP_SENSE_GE (1) or LP_SENSE_EQ (2)";
            return LP_BAD_ARG;
        }
        if (st == lpk::PLAN_GENERAL_BAD_KIND) {
            b->err = who + ", variable " + std::to_string(bad) + ": kind " + std::to_string((int)kind[voff + bad]) +
                     " is not one of LP_VAR_PLAIN (0) to LP_VAR_FREE (4)";
            return LP_BAD_ARG;
        }
        if (st != 0) {
            b->err = who + ": m = " + std::to_string(m[i]) + ", ns = " + std::to_string(ns[i]) + " is no LP's shape";
            return LP_BAD_ARG;
        }
        if (maximise[i] != 0 && maximise[i] != 1) {
            b->err = who + ": maximise " + std::to_string((int)maximise[i]) + " is not 0 or 1";
            return LP_BAD_ARG;
        }
        if (c.rows != b->lp_m(i) || c.cols != b->lp_n(i)) {
            b->err = who + ": its senses and kinds give " + std::to_string(c.rows) + " rows and " +
                     std::to_string(c.cols) + " columns (lp_general_rows, lp_general_columns), the batch has " +
                     std::to_string(b->lp_m(i)) + " and " + std::to_string(b->lp_n(i));
            return LP_BAD_ARG;
        }
        const int64_t xoff = (int64_t)var.size();
        var.resize((size_t)(xoff + c.ns + c.nf));
        (void)lpk::plan_general_tables(sense + yoff, kind + voff, c.m, c.ns, var.data() + xoff, slack.data() + sat,
                                       bvar.data() + sat);
        info[(size_t)i] = lpk::GInfo{poff, xoff, voff, yoff, (int32_t)c.m, (int32_t)c.ns, (int32_t)c.nf, maximise[i]};
        poff += lpk::plan_general_block(c.m, c.ns);
        voff += c.ns;
        yoff += c.m;
        sat += c.rows;
    }
    if (!b->ragged)
        for (int64_t i = 1; i < b->count; ++i) {
            info[(size_t)i] = info[0];
            info[(size_t)i].poff = i * poff, info[(size_t)i].voff = i * voff, info[(size_t)i].yoff = i * yoff;
        }
    const int64_t all = b->ragged ? 1 : b->count;
    info[(size_t)b->count] = lpk::GInfo{all * poff, (int64_t)var.size(), all * voff, all * yoff, 0, 0, 0, 0};
    BCHK(b, hipSetDevice(b->dev));
    b->form_on = false;         // until the tables have landed; the buffers' sizes follow the form
    for (void **p : {(void **)&b->gvar, (void **)&b->gslack, (void **)&b->gbvar, (void **)&b->ginfo,
                     (void **)&b->gstage, (void **)&b->gshift, (void **)&b->gsol, (void **)&b->gdual,
                     (void **)&b->gborder}) {
        if (*p) BCHK(b, hipFree(*p));
        *p = nullptr;
    }
    BCHK(b, hipMalloc(&b->gvar, var.size() * sizeof(lpk::GVar)));
    BCHK(b, hipMalloc(&b->gslack, slack.size() * sizeof(int32_t)));
    BCHK(b, hipMalloc(&b->gbvar, bvar.size() * sizeof(int32_t)));
    BCHK(b, hipMemcpyAsync(b->gvar, var.data(), var.size() * sizeof(lpk::GVar), hipMemcpyHostToDevice, b->s));
    BCHK(b, hipMemcpyAsync(b->gslack, slack.data(), slack.size() * sizeof(int32_t), hipMemcpyHostToDevice, b->s));
    BCHK(b, hipMemcpyAsync(b->gbvar, bvar.data(), bvar.size() * sizeof(int32_t), hipMemcpyHostToDevice, b->s));
    if (b->ragged) {
        BCHK(b, hipMalloc(&b->ginfo, (size_t)b->count * sizeof(lpk::GInfo)));
        BCHK(b, hipMemcpyAsync(b->ginfo, info.data(), (size_t)b->count * sizeof(lpk::GInfo), hipMemcpyHostToDevice,
                               b->s));
    }
    BCHK(b, hipStreamSynchronize(b->s));
    b->hg = std::move(info);
    b->hgvar = std::move(var);
    b->hgslack = std::move(slack);
    b->form_on = true;
    return LP_PIVOTED;
}

extern "C" int lp_general_vars(const lp_batch *b, int64_t index, int64_t *m, int64_t *ns)
{
    if (!b || !m || !ns || !b->form_on) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return LP_BAD_ARG;
    *m = b->hg[(size_t)index].m;
    *ns = b->hg[(size_t)index].ns;
    return LP_PIVOTED;
}

// the window as the four general kernels take it
static lpk::GArgs general_args(const lp_batch *b, int64_t first, int64_t count)
{
    lpk::GArgs A{};
    A.S = solution_args(b, first, count);
    A.out = b->T;
    A.stage = b->gstage;
    A.shift = b->gshift;
    A.var = b->gvar;
    A.slack = b->gslack;
    A.bvar = b->gbvar;
    A.info = b->ragged ? b->ginfo : nullptr;
    A.u = b->hg[0];
    A.u.poff = b->hg[1].poff - b->hg[0].poff;
    A.elems = b->toff(first + count) - b->toff(first);
    return A;
}

// refusals shared by the calls on a live batch; LP_PIVOTED: go on
static int general_window(lp_batch *b, int64_t first, int64_t count)
{
    if (!b->form_on) return bfail(b, "no form attached (lp_general_set_form)");
    return solution_window(b, first, count);
}

extern "C" int lp_general_upload(lp_batch *b, int64_t first, int64_t count, const double *src)
{
    if (!b) return LP_BAD_ARG;
    const int st = general_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (count > 0 && !src) return bfail(b, "host buffer is NULL");
    if (count == 0) return LP_PIVOTED;
    lpk::GArgs A = general_args(b, first, count);
    A.lanes = A.S.nbasis + count;
    const lpk::FlatGrid sgrid = lpk::plan_general_grid(A.lanes), grid = lpk::plan_general_grid(A.elems);
    if (grid.blocks < 0 || sgrid.blocks < 0) return bfail(b, "window too large for one launch: upload it in parts");
    const int64_t at = b->hg[(size_t)first].poff, elems = b->hg[(size_t)(first + count)].poff - at;
    BCHK(b, hipSetDevice(b->dev));
    if (!b->gstage) BCHK(b, hipMalloc(&b->gstage, (size_t)b->hg[(size_t)b->count].poff * sizeof(double)));
    if (!b->gshift) BCHK(b, hipMalloc(&b->gshift, (size_t)(b->boff(b->count) + b->count) * sizeof(double)));
    BCHK(b, hipMemcpyAsync(b->gstage + at, src, (size_t)elems * sizeof(double), hipMemcpyHostToDevice, b->s));
    A.stage = b->gstage;
    A.shift = b->gshift;
    SLAUNCH(b, k_general_shift, sgrid, A);
    SLAUNCH(b, k_general_assemble, grid, A);
    BCHK(b, hipStreamSynchronize(b->s));
    window_reset(b, first, count);
    return LP_PIVOTED;
}

extern "C" int lp_general_solution(lp_batch *b, int64_t first, int64_t count, double *x, double *z)
{
    if (!b) return LP_BAD_ARG;
    const int st = general_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (!b->basis_on) return bfail(b, "no basis attached (lp_batch_set_basis)");
    if (!b->gstage) return bfail(b, "nothing uploaded under this form (lp_general_upload)");
    if (count == 0) return LP_PIVOTED;
    lpk::GArgs A = general_args(b, first, count);
    const int64_t vall = b->hg[(size_t)b->count].voff, v0 = b->hg[(size_t)first].voff;
    const int64_t nv = b->hg[(size_t)(first + count)].voff - v0;
    const lpk::FlatGrid gather = lpk::plan_general_grid(A.S.lanes);
    A.lanes = nv + count;
    const lpk::FlatGrid grid = lpk::plan_general_grid(A.lanes);
    if (gather.blocks < 0 || grid.blocks < 0) return bfail(b, "window too large for one launch: gather it in parts");
    BCHK(b, hipSetDevice(b->dev));
    const int64_t xall = b->coff(b->count);
    if (!b->sol) BCHK(b, hipMalloc(&b->sol, (size_t)(xall + b->count) * sizeof(double)));
    if (!b->gsol) BCHK(b, hipMalloc(&b->gsol, (size_t)(vall + b->count) * sizeof(double)));
    A.S.x = b->sol;
    A.S.z = b->sol + xall;
    A.gx = b->gsol;
    A.gz = b->gsol + vall;
    const lpk::SArgs S = A.S;
    SLAUNCH(b, k_solution, gather, S);
    SLAUNCH(b, k_general_recover, grid, A);
    if (x) BCHK(b, hipMemcpyAsync(x, A.gx + v0, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, b->s));
    if (z) BCHK(b, hipMemcpyAsync(z, A.gz + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

extern "C" int lp_general_duals(lp_batch *b, int64_t first, int64_t count, double *y, double *r)
{
    if (!b) return LP_BAD_ARG;
    const int st = general_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    lpk::GArgs A = general_args(b, first, count);
    const lpk::GInfo &lo = b->hg[(size_t)first], &hi = b->hg[(size_t)(first + count)], &end = b->hg[(size_t)b->count];
    A.rows = hi.yoff - lo.yoff;
    A.lanes = A.rows + (hi.voff - lo.voff);
    const lpk::FlatGrid grid = lpk::plan_general_grid(A.lanes);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: read the duals in parts");
    BCHK(b, hipSetDevice(b->dev));
    if (!b->gdual) BCHK(b, hipMalloc(&b->gdual, (size_t)(end.yoff + end.voff) * sizeof(double)));
    A.gy = b->gdual;
    A.gr = b->gdual + end.yoff;
    SLAUNCH(b, k_general_duals, grid, A);
    if (y) BCHK(b, hipMemcpyAsync(y, A.gy + lo.yoff, (size_t)A.rows * sizeof(double), hipMemcpyDeviceToHost, b->s));
    if (r)
        BCHK(b, hipMemcpyAsync(r, A.gr + lo.voff, (size_t)(hi.voff - lo.voff) * sizeof(double), hipMemcpyDeviceToHost,
                               b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// warm re-optimisation
// ---------------------------------------------------------------------------

extern "C" int lp_reopt_set_costs(lp_batch *b, int64_t first, int64_t count, const double *costs)
{
    if (!b) return LP_BAD_ARG;
    if (!b->basis_on) return bfail(b, "no basis attached (lp_batch_set_basis)");
    const int st = window_ok(b, first, count, costs, b->n + 1);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    // everything is checked on the host first: a refusal copies and launches nothing
    for (int64_t i = first; i < first + count; ++i)
        if (short_rows_refused(b, i)) return LP_BAD_ARG;
    lpk::FArgs A{};
    A.S = solution_args(b, first, count);       // lanes: the window's columns plus one per LP
    A.out = b->T;
    const lpk::FlatGrid grid = lpk::plan_cost_grid(A.S.lanes);
    if (grid.blocks < 0) return bfail(b, "window too large for one launch: set it in parts");
    BCHK(b, hipSetDevice(b->dev));
    if (!b->cost) BCHK(b, hipMalloc(&b->cost, (size_t)(b->coff(b->count) + b->count) * sizeof(double)));
    BCHK(b, hipMemcpyAsync(b->cost, costs, (size_t)A.S.lanes * sizeof(double), hipMemcpyHostToDevice, b->s));
    A.S.x = b->cost;
    SLAUNCH(b, k_cost, grid, A);
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// a bound of the new border that does not fit variable j's kind: the message, and true
static bool bound_refused(lp_batch *b, int64_t i, int64_t j, int kind, double lb, double ub)
{
    static const char *const names[] = {"PLAIN", "LOWER", "BOXED", "UPPER", "FREE"};
    static const char *const needs[] = {"lb == 0 and ub == +inf", "a finite lb and ub == +inf", "both bounds finite",
                                        "lb == -inf and a finite ub", "lb == -inf and ub == +inf"};
    const bool flo = std::isfinite(lb), fhi = std::isfinite(ub);
    bool ok = false;
    if (lb == lb && ub == ub) {
        if (kind == LP_VAR_PLAIN) ok = lb == 0.0 && ub == INFINITY;
        else if (kind == LP_VAR_LOWER) ok = flo && ub == INFINITY;
        else if (kind == LP_VAR_BOXED) ok = flo && fhi;
        else if (kind == LP_VAR_UPPER) ok = lb == -INFINITY && fhi;
        else ok = lb == -INFINITY && ub == INFINITY;
    }
    if (ok) return false;
    b->err = "LP " + std::to_string(i) + ", variable " + std::to_string(j) + ": bounds [" + std::to_string(lb) + ", " +
             std::to_string(ub) + "] do not fit its kind LP_VAR_" + names[kind] + ", which needs " + needs[kind] +
             " (a new pattern of finite bounds is a new form: lp_general_set_form and lp_general_upload)";
    return true;
}

extern "C" int lp_reopt_set_general(lp_batch *b, int64_t first, int64_t count, const double *src)
{
    if (!b) return LP_BAD_ARG;
    const int st = general_window(b, first, count);
    if (st != LP_PIVOTED) return st;
    if (count > 0 && !src) return bfail(b, "host buffer is NULL");
    if (count == 0) return LP_PIVOTED;
    if (!b->gstage) return bfail(b, "nothing uploaded under this form (lp_general_upload)");
    // everything is checked on the host first: a refusal copies and launches nothing
    const double *at = src;
    for (int64_t i = first; i < first + count; ++i) {
        const lpk::GInfo &g = b->hg[(size_t)i];
        if (short_rows_refused(b, i)) return LP_BAD_ARG;
        const int32_t *tab = b->hgslack.data() + (b->ragged ? b->boff(i) : 0);
        for (int64_t r = 0; r < g.m; ++r)
            if (tab[r] == 0) {
                b->err = "LP " + std::to_string(i) + ", row " + std::to_string(r) +
                         " is an equality: it owns no column that holds the basis inverse, as for its dual";
                return LP_BAD_ARG;
            }
        const double *lb = at + g.ns + 1 + g.m, *ub = lb + g.ns;
        for (int64_t j = 0; j < g.ns; ++j)
            if (bound_refused(b, i, j, b->hgvar[(size_t)(g.xoff + j)].kind, lb[j], ub[j])) return LP_BAD_ARG;
        at += lpk::plan_restage_border(g.m, g.ns);
    }
    lpk::GArgs A = general_args(b, first, count);
    const int64_t lanes = at - src, rows = A.S.nbasis + count;
    const lpk::FlatGrid bgrid = lpk::plan_restage_grid(lanes), sgrid = lpk::plan_general_grid(rows);
    if (bgrid.blocks < 0 || sgrid.blocks < 0) return bfail(b, "window too large for one launch: set it in parts");
    BCHK(b, hipSetDevice(b->dev));
    if (!b->gborder) {
        const lpk::GInfo &end = b->hg[(size_t)b->count];
        BCHK(b, hipMalloc(&b->gborder, (size_t)(3 * end.voff + end.yoff + b->count) * sizeof(double)));
    }
    BCHK(b, hipMemcpyAsync(b->gborder, src, (size_t)lanes * sizeof(double), hipMemcpyHostToDevice, b->s));
    A.lanes = lanes;
    const lpk::GBArgs RA{A, b->gborder, b->gstage};
    SLAUNCH(b, k_general_restage, bgrid, RA);
    A.lanes = rows;
    SLAUNCH(b, k_general_shift, sgrid, A);
    // column 0 = M . shift: k_rhs over the m' rows, the shifted column where it reads a staged rhs
    lpk::FArgs R{};
    R.S = A.S;
    R.S.lanes = rows;
    R.S.x = b->gshift + b->boff(first) + first;
    R.out = b->T;
    R.slack = b->gslack;
    SLAUNCH(b, k_rhs, sgrid, R);
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// warm cuts
// ---------------------------------------------------------------------------

// k_cut_copy (0), k_cut_rows (1), k_cut_basis (2): defined at the end of this file, as the two above
static const void *cut_kernel_of(int which);

extern "C" int lp_cut_extend(lp_batch *src, lp_batch *dst, int64_t first, int64_t count, const double *rows,
                             const int8_t *sense)
{
    if (!dst) return LP_BAD_ARG;
    if (!src) return bfail(dst, "the source batch is NULL");
    if (src == dst) return bfail(dst, "the source and the destination are one batch: a batch does not grow in place");
    if (src->dev != dst->dev) return bfail(dst, "the source and the destination are on different devices");
    if (src->count != dst->count) {
        dst->err = "the source holds " + std::to_string(src->count) + " LPs, the destination " +
                   std::to_string(dst->count);
        return LP_BAD_ARG;
    }
    const int st = solution_window(dst, first, count);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    // everything is checked on the host first: a refusal copies and launches nothing
    std::vector<lpk::CutLp> tab((size_t)count + 1);
    lpk::CutLp at{};
    for (int64_t k = 0; k < count; ++k) {
        const int64_t i = first + k, m = src->lp_m(i), n = src->lp_n(i), q = dst->lp_m(i) - m;
        if (q < 0 || dst->lp_n(i) - n != q) {
            dst->err = "LP " + std::to_string(i) + ": the destination's " + std::to_string(dst->lp_m(i)) + " x " +
                       std::to_string(dst->lp_n(i)) + " is not the source's " + std::to_string(m) + " x " +
                       std::to_string(n) + " with q >= 0 more rows and q more columns";
            return LP_BAD_ARG;
        }
        at.stoff = src->toff(i);
        at.dtoff = dst->toff(i);
        at.sboff = src->boff(i);
        at.dboff = dst->boff(i);
        at.m = (int32_t)m;
        at.n = (int32_t)n;
        at.q = (int32_t)q;
        tab[(size_t)k] = at;
        at = lpk::plan_cut_next(at);
    }
    tab[(size_t)count] = at;        // the totals
    const int64_t elems = at.e0, nbasis = at.b0, lanes = at.lane0, nrows = at.roff, nsense = at.qoff;
    if (nsense > 0 && (!rows || !sense)) return bfail(dst, "rows or sense is NULL and some LP gets a row");
    for (int64_t k = 0; k < count; ++k) {
        const lpk::CutLp &L = tab[(size_t)k];
        for (int64_t c = 0; c < L.q; ++c) {
            const int s = sense[L.qoff + c];
            if (s == LP_SENSE_LE || s == LP_SENSE_GE) continue;
            dst->err = "LP " + std::to_string(first + k) + ", row " + std::to_string(c) + " of its new rows: " +
                       (s == LP_SENSE_EQ ? std::string("an equality owns no column: state it as a <= and a >= row")
                                         : "sense " + std::to_string(s) + " is not LP_SENSE_LE (0) or LP_SENSE_GE (1)");
            return LP_BAD_ARG;
        }
    }
    if (!src->basis_on) return bfail(dst, "no basis attached to the source (lp_batch_set_basis)");
    for (int64_t i = first; i < first + count; ++i)
        if (!src->short_rows.empty() && src->short_rows[(size_t)i]) {
            const int64_t live = src->htrec[(size_t)i].rows;
            dst->err = "LP " + std::to_string(i) + ", row " + std::to_string(live) +
                       ": its last two-phase call left " + std::to_string(live) + " of " +
                       std::to_string(src->lp_m(i)) + " rows live";
            return LP_BAD_ARG;
        }
    if (dst->senses_on)
        for (int64_t k = 0; k < count; ++k) {
            const lpk::CutLp &L = tab[(size_t)k];
            const int64_t i = first + k;
            const int32_t *const mine = dst->hslack.data() + (dst->ragged ? dst->boff(i) : 0);
            const int32_t *const theirs =
                src->senses_on ? src->hslack.data() + (src->ragged ? src->boff(i) : 0) : nullptr;
            for (int64_t r = 0; r < L.m + L.q; ++r) {
                const int32_t want = r < L.m ? (theirs ? theirs[r] : mine[r])
                                             : (int32_t)(1 + L.n + (r - L.m)) *
                                                   (sense[L.qoff + (r - L.m)] == LP_SENSE_LE ? 1 : -1);
                if (mine[r] == want) continue;
                dst->err = "LP " + std::to_string(i) + ", row " + std::to_string(r) +
                           ": the destination's senses give it another column than " +
                           (r < L.m ? "the source's senses" : "the sense of this call");
                return LP_BAD_ARG;
            }
        }
    const lpk::FlatGrid cgrid = lpk::plan_cut_copy_grid(elems), rgrid = lpk::plan_cut_grid(lanes),
                        bgrid = lpk::plan_cut_grid(nbasis);
    if (cgrid.blocks < 0 || rgrid.blocks < 0 || bgrid.blocks < 0)
        return bfail(dst, "window too large for one launch: extend it in parts");
    // The launches go to the destination's stream and read the source's buffers.  Every library call
    // returns with its batch's stream drained, so nothing is in flight on the source: no event is needed.
    BCHK(dst, hipSetDevice(dst->dev));
    const size_t tbytes = tab.size() * sizeof(lpk::CutLp), blob = tbytes + (size_t)nsense;
    if (dst->cuttab_cap < (int64_t)blob) {
        if (dst->cuttab) BCHK(dst, hipFree(dst->cuttab));
        dst->cuttab = nullptr;
        dst->cuttab_cap = 0;
        BCHK(dst, hipMalloc(&dst->cuttab, blob));
        dst->cuttab_cap = (int64_t)blob;
    }
    if (dst->cutrows_cap < nrows) {
        if (dst->cutrows) BCHK(dst, hipFree(dst->cutrows));
        dst->cutrows = nullptr;
        dst->cutrows_cap = 0;
        BCHK(dst, hipMalloc(&dst->cutrows, (size_t)nrows * sizeof(double)));
        dst->cutrows_cap = nrows;
    }
    const size_t bbytes = (size_t)dst->boff(dst->count) * sizeof(int32_t);
    if (!dst->basis) BCHK(dst, hipMalloc(&dst->basis, bbytes));
    if (!dst->basis_on) BCHK(dst, hipMemsetAsync(dst->basis, 0xFF, bbytes, dst->s));        // -1 outside the window
    std::vector<unsigned char> host(blob);
    std::memcpy(host.data(), tab.data(), tbytes);
    if (nsense > 0) std::memcpy(host.data() + tbytes, sense, (size_t)nsense);
    BCHK(dst, hipMemcpyAsync(dst->cuttab, host.data(), blob, hipMemcpyHostToDevice, dst->s));
    if (nrows > 0)
        BCHK(dst, hipMemcpyAsync(dst->cutrows, rows, (size_t)nrows * sizeof(double), hipMemcpyHostToDevice, dst->s));
    lpk::CArgs A{};
    A.src = src->T;
    A.sbasis = src->basis;
    A.dst = dst->T;
    A.dbasis = dst->basis;
    A.lp = reinterpret_cast<const lpk::CutLp *>(dst->cuttab);
    A.rows = dst->cutrows;
    A.sense = reinterpret_cast<const int8_t *>(dst->cuttab + tbytes);
    A.count = count;
    A.lanes = elems;
    void *kargs[1] = {&A};
    BCHK(dst, hipLaunchKernel(cut_kernel_of(0), dim3((unsigned)cgrid.blocks), dim3(cgrid.threads), kargs, 0, dst->s));
    if (lanes > 0) {
        A.lanes = lanes;
        BCHK(dst, hipLaunchKernel(cut_kernel_of(1), dim3((unsigned)rgrid.blocks), dim3(rgrid.threads), kargs, 0, dst->s));
    }
    A.lanes = nbasis;
    BCHK(dst, hipLaunchKernel(cut_kernel_of(2), dim3((unsigned)bgrid.blocks), dim3(bgrid.threads), kargs, 0, dst->s));
    BCHK(dst, hipStreamSynchronize(dst->s));
    dst->basis_on = true;
    window_reset(dst, first, count);
    return LP_PIVOTED;
}

extern "C" int lp_batch_log(lp_batch *b, int64_t index, int64_t *rc, int64_t cap, int64_t *count)
{
    if (!b) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return bfail(b, "LP index out of bounds");
    if (cap < 0 || (cap > 0 && !rc)) return bfail(b, "bad log buffer");
    const int64_t all = b->nlog.empty() ? b->hrec[(size_t)index].npiv : b->nlog[(size_t)index];
    if (count) *count = all;
    const int64_t kept = std::min(all, b->log ? b->logcap : (int64_t)0);
    const int64_t take = std::min(kept, cap);
    if (take > 0) {
        static_assert(sizeof(long long) == sizeof(int64_t), "log entries are 64-bit");
        BCHK(b, hipSetDevice(b->dev));
        BCHK(b, hipMemcpyAsync(rc, b->log + (size_t)index * (size_t)b->logcap * 2,
                               (size_t)take * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, b->s));
        BCHK(b, hipStreamSynchronize(b->s));
    }
    return LP_PIVOTED;
}

// ---------------------------------------------------------------------------
// two-phase solve
// ---------------------------------------------------------------------------

// (m+1) x (n+1+m) live elements up to here: one wave per LP, four above -- the
// threshold of the plain batch kernel applied to the widest artificial problem
static int twophase_waves(int64_t m, int64_t n)
{
    return (m + 1) * (n + 1 + m) <= BATCH_ONE_WAVE_ELEMS ? 1 : 4;
}

// lp_batch_create's formula at the widened pitch (n+1+m) | 1, plus the basis
// (m int32) kept in LDS
extern "C" int64_t lp_twophase_lds_bytes(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0) return LP_BAD_ARG;
    if (m >= (1 << 20) || n >= (1 << 20)) return INT64_MAX;
    const int64_t pitch = (n + 1 + m) | 1;
    return ((m + 1) * pitch + pitch + (m + 1) + 16 + (m + 1) / 2) * 8;
}

// lp_twophase_solve (phased = false) and lp_phased_solve on a batch whose
// placement lets an LP run from device memory (phased = true): the same
// records, buffers, relaunch loop and report; what differs is the plan the
// launches come from
static int twophase_run(lp_batch *b, bool phased, int64_t max_pivots, int32_t *status, int32_t *stage,
                        int64_t *rows, int64_t *ninit, int64_t *npiv, int64_t *nstd)
{
    const int64_t m = b->m, n = b->n, ww = n + 1 + m;
    if (phased) {           // refuses an LP that is too large for either placement, before any launch
        const int st = ensure_plan(b, 2);
        if (st != LP_PIVOTED) return st;
        // a uniform batch is one bin: in LDS it is the two-phase call itself
        if (!b->ragged && !b->plan[2].bins[0].device) phased = false;
    }
    const int tp = phased ? 2 : 1;      // the plan a ragged batch launches from
    const int64_t lds = b->ragged ? 0 : phased ? b->plan[2].bins[0].lds : lp_twophase_lds_bytes(m, n);
    if (lds > (int64_t)BATCH_LDS_MAX)
        return bfail(b, "shape too large for the two-phase batch path: (m+1) x (n+1+m) float64 plus "
                        "its side buffers must fit one CU's 160 KiB of LDS (use Simplex per LP)");
    const int waves = b->ragged ? 0 : twophase_waves(m, n);
    if (b->ragged && !phased) {     // refuses an LP that is too large, with its index, before any launch
        const int st = ensure_plan(b, 1);
        if (st != LP_PIVOTED) return st;
    }
    BCHK(b, hipSetDevice(b->dev));
    if (!b->trec && b->ragged) {
        if (!b->W) BCHK(b, hipMalloc(&b->W, (size_t)b->woff(b->count) * sizeof(double)));
        if (!b->origc) BCHK(b, hipMalloc(&b->origc, (size_t)b->coff(b->count) * sizeof(double)));
        if (!b->basis) BCHK(b, hipMalloc(&b->basis, (size_t)b->boff(b->count) * sizeof(int32_t)));
        BCHK(b, hipMalloc(&b->trec, (size_t)b->count * sizeof(TRec)));
    }
    if (!b->ragged && !phased && !b->tp_attr) {     // (the phased plan has checked and set its own kernel's)
        int granted = 0;
        int st = lds_granted(b, &granted);
        if (st == LP_PIVOTED)
            st = lds_grant(b, granted, {K_TWOPHASE, false, waves}, lds,
                           "shape too large for the two-phase batch path on this device" + lds_needs(lds, granted));
        if (st != LP_PIVOTED) return st;
        b->tp_attr = true;
    }
    if (!b->trec) {
        const size_t cnt = (size_t)b->count;
        if (!b->W) BCHK(b, hipMalloc(&b->W, cnt * (size_t)(m + 1) * (size_t)ww * sizeof(double)));
        if (!b->origc) BCHK(b, hipMalloc(&b->origc, cnt * (size_t)n * sizeof(double)));
        if (!b->basis) BCHK(b, hipMalloc(&b->basis, cnt * (size_t)m * sizeof(int32_t)));
        BCHK(b, hipMalloc(&b->trec, cnt * sizeof(TRec)));
    }
    const size_t rbytes = (size_t)b->count * sizeof(BRec), tbytes = (size_t)b->count * sizeof(TRec);
    b->hrec.assign((size_t)b->count, BRec{});        // B_START
    b->htrec.assign((size_t)b->count, TRec{});
    b->nlog.assign((size_t)b->count, 0);
    b->basis_on = true;                              // derived here; replaces an attached one
    BCHK(b, hipMemcpyAsync(b->rec, b->hrec.data(), rbytes, hipMemcpyHostToDevice, b->s));
    BCHK(b, hipMemcpyAsync(b->trec, b->htrec.data(), tbytes, hipMemcpyHostToDevice, b->s));
    TArgs A{};
    A.B.T = b->T;
    A.B.rec = b->rec;
    A.B.log = b->log;
    A.B.basis = b->basis;
    A.B.count = b->count;
    A.B.logcap = b->log ? b->logcap : 0;
    A.B.chunk = b->chunk;
    A.B.limit = max_pivots < 0 ? -1 : max_pivots;
    A.B.m = (int)m;
    A.B.n = (int)n;
    A.B.pitch = (int)(ww | 1);
    A.B.mode = lpk::MODE_SOLVE;
    A.B.tol = b->tol;
    A.W = b->W;
    A.origc = b->origc;
    A.trec = b->trec;
    A.ww = (int)ww;
    const UniformLaunch U{(size_t)lds, phased, waves};
    const int st = drive(b, false, [&]() -> int {
        return b->ragged ? launch_unfinished<lpk::PArgs, true>(b, tp, K_TWOPHASE, K_PHASED, false, false, A, U)
                         : launch_unfinished<lpk::PArgs, false>(b, tp, K_TWOPHASE, K_PHASED, false, false, A, U);
    });
    if (st != LP_PIVOTED) return st;
    BCHK(b, hipMemcpyAsync(b->htrec.data(), b->trec, tbytes, hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    b->short_rows.assign((size_t)b->count, 0);
    for (int64_t i = 0; i < b->count; ++i) {
        const BRec &r = b->hrec[(size_t)i];
        const TRec &t = b->htrec[(size_t)i];
        const bool p2 = t.stage == LP_STAGE_PHASE2;
        b->short_rows[(size_t)i] = t.rows < b->lp_m(i) ? 1 : 0;
        b->nlog[(size_t)i] = t.ninit + (p2 ? r.npiv : 0);
        if (status) status[i] = r.status;
        if (stage) stage[i] = t.stage;
        if (rows) rows[i] = t.rows;
        if (ninit) ninit[i] = t.ninit;
        if (npiv) npiv[i] = p2 ? r.npiv : 0;
        if (nstd) nstd[i] = p2 ? r.nstd : 0;
    }
    return 0;
}

extern "C" int lp_twophase_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int32_t *stage,
                                 int64_t *rows, int64_t *ninit, int64_t *npiv, int64_t *nstd)
{
    if (!b) return LP_BAD_ARG;
    return twophase_run(b, false, max_pivots, status, stage, rows, ninit, npiv, nstd);
}

// lp_twophase_solve with each LP placed by plan_place_phased under the batch's
// creation-time placement; on an LP_PLACE_LDS batch it is lp_twophase_solve
extern "C" int lp_phased_solve(lp_batch *b, int64_t max_pivots, int32_t *status, int32_t *stage,
                               int64_t *rows, int64_t *ninit, int64_t *npiv, int64_t *nstd)
{
    if (!b) return LP_BAD_ARG;
    return twophase_run(b, b->place != LP_PLACE_LDS, max_pivots, status, stage, rows, ninit, npiv, nstd);
}

// ---- LP_RULE_MAX_INCREASE's instantiations, last in the file: see the declaration
static const void *maxinc_kernel_of(const KKey &k)
{
    using namespace lpk;
    static const void *const K[2][3] = {             // [ragged][device, one wave, four waves]
        {(const void *)&k_batch_dev<BATCH_DEV_WAVES, false, true>, (const void *)&k_batch<1, false, true>,
         (const void *)&k_batch<4, false, true>},
        {(const void *)&k_batch_dev<BATCH_DEV_WAVES, true, true>, (const void *)&k_batch<1, true, true>,
         (const void *)&k_batch<4, true, true>}};
    return K[k.ragged ? 1 : 0][k.family == K_DEVICE ? 0 : k.waves == 1 ? 1 : 2];
}

// ---- LP_RULE_DUAL's instantiations, after those: the same reason
static const void *dual_kernel_of(const KKey &k)
{
    using namespace lpk;
    static const void *const K[2][3] = {             // [ragged][device, one wave, four waves]
        {(const void *)&k_batch_dev<BATCH_DEV_WAVES, false, false, true>, (const void *)&k_batch<1, false, false, true>,
         (const void *)&k_batch<4, false, false, true>},
        {(const void *)&k_batch_dev<BATCH_DEV_WAVES, true, false, true>, (const void *)&k_batch<1, true, false, true>,
         (const void *)&k_batch<4, true, false, true>}};
    return K[k.ragged ? 1 : 0][k.family == K_DEVICE ? 0 : k.waves == 1 ? 1 : 2];
}

// ---- the warm cuts' kernels, after those: see their declarations
namespace lpk {
namespace {

// lanes over the window's destination elements, PLAN_ASSEMBLE_RUN consecutive
// ones each: a copied cell, +0.0 or +1.0; the cells of the priced rows are
// k_cut_rows'.  Adjacent lanes copy adjacent cells of a row.
template <int RUN>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_cut_copy(const CArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    const CutLp *const lp = A.lp;
    const double *const src = A.src;
    double *const dst = A.dst;
    const long long count = A.count;
    plan_cut_lane(
        g * RUN, A.lanes,
        [=](long long e) { return plan_lane_lp(0, count, e, [=](long long k) { return lp[k].e0; }); },
        [=](long long k) { return lp[k]; },
        [=](long long to, int kind, long long from) {
            if (kind == PLAN_CUT_PRICED) return;
            dst[to] = kind == PLAN_CUT_COPY ? src[from] : kind == PLAN_CUT_ONE ? 1.0 : 0.0;
        });
}

// the priced rows: a lane is one (LP, group of up to PLAN_CUT_GROUP new rows,
// source column j) triple and walks column j of the source rows once, r
// ascending, one accumulator per row of its group.  Adjacent lanes read
// adjacent cells of a row; the basis entry and the stated coefficient are the
// same address across a group's lanes.
template <int GROUP>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_cut_rows(const CArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const CutLp *const lp = A.lp;
    const CutLp L = lp[plan_lane_lp(0, A.count, g, [=](long long k) { return lp[k].lane0; })];
    const CutAt at = plan_cut_at(g - L.lane0, L.n);
    const int w = L.n + 1, k1 = min(L.q, at.k0 + GROUP);
    const long long dw = w + L.q;
    const double *const col = A.src + L.stoff + w + at.col;        // T[1][j]
    const int32_t *const basis = A.sbasis + L.sboff;
    const double *const rows = A.rows + L.roff;
    const int8_t *const sense = A.sense + L.qoff;
    double *const out = A.dst + L.dtoff + (1 + L.m) * dw + at.col;     // D[1+m][j]
    plan_cut_rows<GROUP>(
        at.col, L.m, L.n, at.k0, k1, [=](int r) { return (int)basis[r]; },
        [=](int r) { return col[(long long)r * w]; }, [=](int k, int c) { return rows[(long long)k * w + c]; },
        [=](int k, double acc) { out[k * dw] = sense[k] == PLAN_SENSE_GE ? plan_cut_flip(acc) : acc; });
}

// the destination basis: lanes over the window's destination basis entries,
// the source's m entries, then n + k for new row k
template <int RUN>
__global__ __launch_bounds__(PLAN_FLAT_THREADS) void k_cut_basis(const CArgs A)
{
    const long long g = (long long)blockIdx.x * PLAN_FLAT_THREADS + threadIdx.x;
    if (g >= A.lanes) return;
    const CutLp *const lp = A.lp;
    const CutLp L = lp[plan_lane_lp(0, A.count, g, [=](long long k) { return lp[k].b0; })];
    const int r = (int)(g - L.b0);
    A.dbasis[L.dboff + r] = r < L.m ? A.sbasis[L.sboff + r] : L.n + (r - L.m);
}

}  // namespace
}  // namespace lpk

static const void *cut_kernel_of(int which)
{
    using namespace lpk;
    static const void *const K[3] = {(const void *)&k_cut_copy<PLAN_ASSEMBLE_RUN>,
                                     (const void *)&k_cut_rows<PLAN_CUT_GROUP>, (const void *)&k_cut_basis<1>};
    return K[which];
}
