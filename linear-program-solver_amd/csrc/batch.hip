// Batched solve: many small LPs of one shape, one workgroup per LP, the LP's
// whole (m+1) x (n+1) float64 tableau in LDS for the life of a launch
// (lp_batch_* in include/lpgpu.h; DESIGN.md "Batched solve").
//
// The float semantics are the header comment of oracle/lp_f64.c, pivot for
// pivot; the solve logic is lpf_solve / lpf_run restated per LP.  There is no
// communication between workgroups and no waiting of any kind: a launch runs
// at most `chunk` pivots per LP, leaves each LP's state in a small global
// record, and the host relaunches while any LP is still in progress.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device.h"

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
    int32_t pad;
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

// LDS: tableau rows at `pitch` doubles (odd: the ratio test reads a column,
// lanes over rows, 2*pitch dwords apart -- distinct banks mod 64 per 32-lane
// half), then the normalised pivot row P (pitch), the multipliers F (m+1) and
// the reduction scratch (16).
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_batch(const BArgs A)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ double lds[];
    const long long lp = blockIdx.x;
    if (lp >= A.count) return;
    BRec *const rp = A.rec + lp;
    const int state = rp->state;
    if (state == B_DONE) return;            // block-uniform: every thread reads the same record

    const int tid = threadIdx.x;
    const int m = A.m, n = A.n, w = A.n + 1, pitch = A.pitch;
    const int E = (m + 1) * w;
    double *const Tl = lds;
    double *const Pl = Tl + (size_t)(m + 1) * pitch;
    double *const Fl = Pl + pitch;
    double *const sc = Fl + (m + 1);
    double *const Tg = A.T + lp * (long long)E;
    const lp_tol tol = A.tol;
    // element e = i * w + j walked with a stride of NT, (i, j) carried along
    const int di = NT / w, dj = NT % w, i0 = tid / w, j0 = tid % w;

    {
        int i = i0, j = j0;
        for (int e = tid; e < E; e += NT) {
            Tl[i * pitch + j] = Tg[e];
            j += dj;
            i += di;
            if (j >= w) { j -= w; ++i; }
        }
    }
    __syncthreads();

    long long npiv, nstd, stuck;
    double z0;
    int rule;
    if (state == B_START) {
        npiv = nstd = stuck = 0;
        z0 = -Tl[0];
        rule = A.mode == MODE_SOLVE ? (int)LP_RULE_STANDARD : A.run_rule;
    } else {
        npiv = rp->npiv;
        nstd = rp->nstd;
        stuck = rp->stuck;
        z0 = rp->z0;
        rule = rp->rule;
    }
    const long long npiv_in = npiv;
    int status = LP_PIVOTED;
    bool done = false;

    // Every exit below is taken from block-reduced or LDS-resident values that
    // all threads read identically, so the barriers inside stay uniform.
    for (long long it = 0; it < A.chunk; ++it) {
        if (A.mode == MODE_SOLVE && rule == LP_RULE_STANDARD && stuck >= (long long)m + n)
            rule = LP_RULE_MIN_INDEX;
        if (A.limit >= 0 && npiv >= A.limit) {      // before the selection, as lpf_solve
            status = A.mode == MODE_SOLVE ? LP_CAP_REACHED : LP_PIVOTED;
            done = true;
            break;
        }

        // ---- entering column (entering() in lp_f64.c)
        long long k = NONE;
        if (rule == LP_RULE_MIN_INDEX) {
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
        const long long C = bmin_ll<WAVES>(k, sc);
        if (C == NONE) {
            status = LP_OPTIMAL;
            done = true;
            break;
        }

        // ---- ratio test (leaving() in lp_f64.c): eligibility is a flag, the
        // minimum starts at the first eligible row's ratio (a NaN there stays),
        // the band g + tie |g| is not clamped
        double v = INFINITY;
        long long fe = NONE;
        for (int i = 1 + tid; i <= m; i += NT) {
            bool ok;
            const double q = row_ratio(Tl[i * pitch + C], Tl[i * pitch], tol, ok);
            if (ok) {
                v = fmin(v, q);
                if (fe == NONE) fe = 2LL * i + (q != q ? 1 : 0);
            }
        }
        double g = bmin<WAVES>(v, sc);
        fe = bmin_ll<WAVES>(fe, sc);
        if (fe == NONE) {
            status = LP_UNBOUNDED;
            done = true;
            break;
        }
        if (fe & 1) g = NAN;
        const double thr = g + tol.ratio_tie * fabs(g);
        k = NONE;
        for (int i = 1 + tid; i <= m; i += NT) {
            bool ok;
            const double q = row_ratio(Tl[i * pitch + C], Tl[i * pitch], tol, ok);
            if (ok && q <= thr && k == NONE) k = i;
        }
        const long long R = bmin_ll<WAVES>(k, sc);
        if (R == NONE) {                    // lp_f64.c's "unreachable" -1 (a NaN band)
            status = LP_UNBOUNDED;
            done = true;
            break;
        }

        // ---- pivot (lpf_pivot): save the multipliers and the normalised row,
        // then one pass of FMAs over the whole tableau
        const double a = Tl[R * pitch + C];
        if (a != 0.0) {                     // lpf_solve counts a zero pivot without applying it
            for (int i = tid; i <= m; i += NT) Fl[i] = Tl[i * pitch + C];
            for (int j = tid; j <= n; j += NT) Pl[j] = j == C ? 1.0 : Tl[R * pitch + j] / a;
            __syncthreads();
            int i = i0, j = j0;
            for (int e = tid; e < E; e += NT) {
                const double x = Tl[i * pitch + j];
                Tl[i * pitch + j] = upd(i, R, Fl[i], Pl[j], x);
                j += dj;
                i += di;
                if (j >= w) { j -= w; ++i; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (A.basis) A.basis[lp * m + (R - 1)] = (int32_t)(C - 1);
            if (npiv < A.logcap) {
                long long *const l = A.log + (lp * A.logcap + npiv) * 2;
                l[0] = R - 1;
                l[1] = C - 1;
            }
        }
        ++npiv;
        if (A.mode == MODE_SOLVE && rule == LP_RULE_STANDARD) {
            ++nstd;
            const double z = -Tl[0];
            const double band = tol.stall * fmax(1.0, fabs(z0));
            if (z - z0 > band) {
                status = LP_OBJ_INCREASED;  // after the offending pivot
                done = true;
                break;
            }
            if (fabs(z - z0) <= band) ++stuck;
            else stuck = 0;
        }
    }

    if (npiv != npiv_in) {
        int i = i0, j = j0;
        for (int e = tid; e < E; e += NT) {
            Tg[e] = Tl[i * pitch + j];
            j += dj;
            i += di;
            if (j >= w) { j -= w; ++i; }
        }
    }
    if (tid == 0) {
        rp->status = status;
        rp->state = done ? B_DONE : B_RUNNING;
        rp->rule = rule;
        rp->npiv = npiv;
        rp->nstd = nstd;
        rp->stuck = stuck;
        rp->z0 = z0;
    }
}

}  // namespace
}  // namespace lpk

using lpk::BArgs;
using lpk::BRec;

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct lp_batch {
    int dev = 0;
    hipStream_t s = nullptr;
    int64_t count = 0, m = 0, n = 0, logcap = 0, chunk = 4096;
    int pitch = 0, waves = 1;
    size_t lds = 0;
    double *T = nullptr;
    BRec *rec = nullptr;
    long long *log = nullptr;
    int32_t *basis = nullptr;
    bool basis_on = false;
    lp_tol tol{};
    std::vector<BRec> hrec;
    std::string err;
};

static std::string g_batch_err;

constexpr size_t BATCH_LDS_MAX = 160u * 1024u;      // one CU's LDS
// (m+1)(n+1) up to here: one wave per LP, four above (DESIGN.md "Batched solve";
// the A/B builds of scripts/batch_waves.py move it with -DLPGPU_BATCH_ONE_WAVE_ELEMS=)
#ifndef LPGPU_BATCH_ONE_WAVE_ELEMS
#define LPGPU_BATCH_ONE_WAVE_ELEMS 2048
#endif
constexpr int64_t BATCH_ONE_WAVE_ELEMS = LPGPU_BATCH_ONE_WAVE_ELEMS;

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

static const void *batch_kernel(int waves)
{
    return waves == 1 ? reinterpret_cast<const void *>(&lpk::k_batch<1>)
                      : reinterpret_cast<const void *>(&lpk::k_batch<4>);
}

static int batch_alloc(lp_batch *b)
{
    BCHK(b, hipSetDevice(b->dev));
    int granted = 0;
    BCHK(b, hipDeviceGetAttribute(&granted, hipDeviceAttributeMaxSharedMemoryPerBlock, b->dev));
    if (b->lds > (size_t)granted) {
        b->err = "shape too large for the batch path on this device: needs " +
                 std::to_string(b->lds) + " bytes of LDS per workgroup, the device grants " +
                 std::to_string(granted) + " (use lp_create)";
        return LP_BAD_ARG;
    }
    if (b->lds > 64u * 1024u)
        BCHK(b, hipFuncSetAttribute(batch_kernel(b->waves), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)b->lds));
    BCHK(b, hipStreamCreateWithFlags(&b->s, hipStreamNonBlocking));
    const size_t elems = (size_t)b->count * (size_t)(b->m + 1) * (size_t)(b->n + 1);
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
    if (b->s || b->T || b->rec || b->log || b->basis) {
        (void)hipSetDevice(b->dev);
        if (b->s) (void)hipStreamSynchronize(b->s);
        if (b->T) (void)hipFree(b->T);
        if (b->rec) (void)hipFree(b->rec);
        if (b->log) (void)hipFree(b->log);
        if (b->basis) (void)hipFree(b->basis);
        if (b->s) (void)hipStreamDestroy(b->s);
    }
    delete b;
    return LP_PIVOTED;
}

extern "C" int lp_batch_create(int64_t count, int64_t m, int64_t n, int64_t log_cap, int device,
                               lp_batch **out)
{
    if (!out) {
        g_batch_err = "out is NULL";
        return LP_BAD_ARG;
    }
    *out = nullptr;
    if (count <= 0 || m <= 0 || n <= 0 || log_cap < 0) {
        g_batch_err = "need count > 0, m > 0, n > 0 and log_cap >= 0";
        return LP_BAD_ARG;
    }
    // (m+1) rows at an odd pitch + P (pitch) + F (m+1) + 16 of scratch, in doubles
    const int64_t pitch = (n + 1) | 1;
    const bool small = m < (1 << 20) && n < (1 << 20);
    const int64_t need = small ? ((m + 1) * pitch + pitch + (m + 1) + 16) * 8 : INT64_MAX;
    if (need > (int64_t)BATCH_LDS_MAX) {
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
    b->waves = (m + 1) * (n + 1) <= BATCH_ONE_WAVE_ELEMS ? 1 : 4;
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
    if (ldh < b->n + 1) return bfail(b, "ldh < n + 1");
    return LP_PIVOTED;
}

extern "C" int lp_batch_upload(lp_batch *b, int64_t first, int64_t count, const double *src,
                               int64_t ldh)
{
    if (!b) return LP_BAD_ARG;
    const int st = window_ok(b, first, count, src, ldh);
    if (st != LP_PIVOTED) return st;
    if (count == 0) return LP_PIVOTED;
    const size_t w = (size_t)(b->n + 1) * sizeof(double), rows = (size_t)(b->m + 1);
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpy2DAsync(b->T + (size_t)first * rows * (size_t)(b->n + 1), w, src,
                             (size_t)ldh * sizeof(double), w, (size_t)count * rows,
                             hipMemcpyHostToDevice, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    for (int64_t i = first; i < first + count; ++i) b->hrec[(size_t)i] = BRec{};
    return LP_PIVOTED;
}

extern "C" int lp_batch_download(lp_batch *b, int64_t first, int64_t count, double *dst, int64_t ldh)
{
    if (!b) return LP_BAD_ARG;
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

extern "C" int lp_batch_set_basis(lp_batch *b, const int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (!basis) {
        b->basis_on = false;
        return LP_PIVOTED;
    }
    const size_t bytes = (size_t)b->count * (size_t)b->m * sizeof(int32_t);
    BCHK(b, hipSetDevice(b->dev));
    if (!b->basis) BCHK(b, hipMalloc(&b->basis, bytes));
    BCHK(b, hipMemcpyAsync(b->basis, basis, bytes, hipMemcpyHostToDevice, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    b->basis_on = true;
    return LP_PIVOTED;
}

extern "C" int lp_batch_get_basis(lp_batch *b, int32_t *basis)
{
    if (!b) return LP_BAD_ARG;
    if (!basis) return bfail(b, "basis is NULL");
    if (!b->basis_on) return bfail(b, "no basis attached (lp_batch_set_basis)");
    const size_t bytes = (size_t)b->count * (size_t)b->m * sizeof(int32_t);
    BCHK(b, hipSetDevice(b->dev));
    BCHK(b, hipMemcpyAsync(basis, b->basis, bytes, hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    return LP_PIVOTED;
}

// One lpf_solve / lpf_run per LP: bounded launches until every record is done.
static int batch_drive(lp_batch *b, int mode, int rule, int64_t limit)
{
    BCHK(b, hipSetDevice(b->dev));
    const size_t rbytes = (size_t)b->count * sizeof(BRec);
    b->hrec.assign((size_t)b->count, BRec{});        // B_START
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
    const dim3 grid((unsigned)b->count);
    for (;;) {
        if (b->waves == 1)
            hipLaunchKernelGGL(lpk::k_batch<1>, grid, dim3(64), b->lds, b->s, A);
        else
            hipLaunchKernelGGL(lpk::k_batch<4>, grid, dim3(256), b->lds, b->s, A);
        BCHK(b, hipGetLastError());
        BCHK(b, hipMemcpyAsync(b->hrec.data(), b->rec, rbytes, hipMemcpyDeviceToHost, b->s));
        BCHK(b, hipStreamSynchronize(b->s));
        bool more = false;
        for (const BRec &r : b->hrec)
            if (r.state != lpk::B_DONE) {
                more = true;
                break;
            }
        if (!more) return LP_PIVOTED;
    }
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
    if (rule != LP_RULE_STANDARD && rule != LP_RULE_MIN_INDEX) return bfail(b, "unknown rule");
    if (k < 0) return bfail(b, "k < 0");
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
    const size_t lp_bytes = (size_t)(b->m + 1) * (size_t)(b->n + 1) * sizeof(double);
    BCHK(b, hipMemcpy2DAsync(z, sizeof(double), b->T, lp_bytes, sizeof(double), (size_t)b->count,
                             hipMemcpyDeviceToHost, b->s));
    BCHK(b, hipStreamSynchronize(b->s));
    for (int64_t i = 0; i < b->count; ++i) z[i] = -z[i];
    return LP_PIVOTED;
}

extern "C" int lp_batch_log(lp_batch *b, int64_t index, int64_t *rc, int64_t cap, int64_t *count)
{
    if (!b) return LP_BAD_ARG;
    if (index < 0 || index >= b->count) return bfail(b, "LP index out of bounds");
    if (cap < 0 || (cap > 0 && !rc)) return bfail(b, "bad log buffer");
    const int64_t all = b->hrec[(size_t)index].npiv;
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
