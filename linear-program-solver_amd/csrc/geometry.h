// Launch planning: which kernel, which grid, how the rows and columns are
// dealt out.  Pure functions of the shape, the knobs (knobs.h, as arguments)
// and the occupancy the caller found: no planner reads the environment or the
// device and nothing here needs HIP, so all of it runs on a CPU
// (csrc/geometry_check.cpp, tests/test_geometry_cpu.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>

#ifdef __HIP__
#define LPK_HD __host__ __device__
#else
#define LPK_HD
#endif

namespace lpk {

constexpr int BMAX = 64;           // most pivots deferred into one sweep

constexpr int GROUP_MAXBLOCKS = 256;
constexpr int XS_SHARDS = 8;          // XCD shards of one device (MI355X: 8 XCDs)
constexpr int GROUP_MINBLOCKS = 64;    // a small tableau still spreads its columns over 64 blocks
constexpr int GROUP_THREADS = 64;      // one wave: block reductions stay in registers
constexpr int GROUP_MAXRPL = 4;        // own rows per lane (<= 64 x 256 x 4 = 65536 rows per device, as LDS allows)
constexpr long long GROUP_LDS_MAX = 96 * 1024;
// dynamic LDS of one k_group block: per own row / own column the pivots'
// values at stride count + 1 (multipliers, pivot-row values) + row 0 /
// column 0 slices
LPK_HD inline long long group_lds(long long rc, long long ld, long long g, int count)
{
    const long long rpb = (rc + g - 1) / g, cpb = (ld + g - 1) / g;
    return ((rpb + cpb) * (count + 1) + cpb + rpb + 8) * 8;   // + a chunk of slack
}

// k_group's compiled variants (summaries per lane, columns per lane, rows per lane)
#define GROUP_VARIANTS(X) \
    X(1, 2, 1) X(2, 2, 1) X(4, 2, 1) X(1, 3, 1) X(2, 3, 1) X(1, 4, 1) X(2, 4, 1) X(4, 4, 1) X(4, 2, 2) X(4, 4, 2) \
        X(4, 2, 4) X(4, 4, 4)

// Geometry of one persistent selection launch (k_group), decided on the host
// from the compiled kernel's occupancy (group_geom, kernels.hip).  g == 0:
// the shape does not fit (the per-pivot kernels are used instead).
struct GroupGeom {
    long long g = 0;     // workgroups (one wave each) per shard
    int nr = 1;          // summaries per lane (g <= 64 nr)
    int ipl = 2;         // own columns per lane (cpb <= 64 ipl)
    int rpl = 1;         // own rows per lane (rpb <= 64 rpl)
    int xmode = 0;       // 1: every block on ONE XCD (grid 8 g, blocks 0, 8, 16, ...)
    int hk = 0;          // 1: blocks spread over the XCDs, the k_group variant with the two-level exchange
    size_t lds = 0;      // dynamic LDS per block
    int per_cu = 0;      // resident blocks per CU the launch relies on
    int sel = 0;         // > 0: the one-XCD selection k_sel (select.hip) for up to `sel` pivots per launch
    int xs = 0;          // > 0: k_sel split into `xs` row shards, one per XCD, in one launch (g blocks each)
};

// ---- the tableau's row pitch -----------------------------------------------
// Row pitch of the tableau in doubles: a multiple of 64 (512 B: rows start
// on a cache line, 16-byte accesses stay aligned) that holds n + 1 columns
// and is not "aliased".  A pitch of p x 512 B where p x d lies within
// 1.5 min(k, 3) of k x 128 (k x 64 KiB) for some d = 1..4 sends the
// selection's column gather -- one element from each of 32768 rows -- to few
// HBM channels, at about twice the time of its neighbours
// (scripts/gather_probe.hip, profiles/r02/gather_pitch.json: 3.6 us against
// 1.7 us at p = 127/129 and 4.1 / 3.8 at 254 / 258; 2.2-2.6 at 43, 64, 86,
// 172).  cfg3 / cfg4 (n = 8192): p = 129 -> 130.  At most 16 steps up.
inline bool pitch_aliased(int64_t p)
{
    for (int64_t d = 1; d <= 4; ++d) {
        const int64_t q = p * d, k = (q + 64) / 128;
        if (k < 1) continue;
        const int64_t dist = q > 128 * k ? q - 128 * k : 128 * k - q;
        if (2 * dist <= 3 * std::min<int64_t>(k, 3)) return true;
    }
    return false;
}

// raw (LPGPU_LD_RAW=1, A/B): the plain rounded pitch
inline int64_t row_pitch(int64_t n, bool raw)
{
    const int64_t p0 = (n + 1 + 63) / 64;
    if (raw || p0 < 16) return p0 * 64;
    for (int64_t p = p0; p < p0 + 16; ++p)
        if (!pitch_aliased(p)) return p * 64;
    return p0 * 64;
}

// ---- the sweep ---------------------------------------------------------------
struct SweepShape {
    long long rows, n, ld;   // Args::rows, n, ld
    int nd_max;              // the handle's pivots per sweep
    int cnt;                 // (> 0) the most pivots this group can hold, when the host knows it
    int share;               // Args::share
    bool second_buffer;      // the handle has another tableau buffer (A.Tout != A.T)
};
struct SweepEnv {
    int cus;                 // the CUs the grid is sized for (all, or LPGPU_SWEEP_CUS)
    int bpc;                 // resident workgroups per CU of the chosen kernel
    int tail_mode;           // LPGPU_SWEEP_TAIL: 0 no tail piece (a strip of its own), 2 k_sweep_dp2's at any length
    double split;            // LPGPU_SWEEP_SPLIT (default SWEEP_SPLIT; 0: equal runs)
};
struct SweepKernel {
    bool rl = false;         // k_sweep_rl<W, 64, D, SA | 2 oop>, else k_sweep_dp2<10, nb, SA>
    int W = 10, D = 0;       // waves per workgroup; batches in flight (rl)
    bool oop = false;        // rl: out of place, into the handle's other buffer
    int nb = 64;             // the kernel's depth
    int nexp = 64;           // rl: pivots the group holds; the host zero-fills the rest of nb before the launch
};
struct SweepPlan {
    SweepKernel k;
    long long nsg = 0, nrun = 0;   // column strips with blocks of their own, row runs per strip
    long long run = 0, runb = 0;   // rows of runs 0 .. na - 1, of the rest
    int na = 0;
    long long tail = 0;            // rows of the tail piece per block (0: none)
    long long tcol = 0, tend = 0;  // rl: the tail piece's first column, one past the last column
    long long grid = 0;
};

// k_sweep_rl for groups of 49..64 pivots (the automatic depth of cfg3 and
// cfg4 is 64, so it is the bench's kernel), k_sweep_dp2 for up to 48 (and
// every tableau narrower than two 64-column strips).
inline SweepKernel choose_sweep_kernel(const SweepShape &S)
{
    SweepKernel K;
    // the kernel's depth: the group's known pivot count when the host knows it
    // (a call's last group, explicit pivots), else the handle's depth
    int nd_max = S.nd_max;
    if (S.cnt > 0 && S.cnt < nd_max) nd_max = S.cnt;
    const int nb = nd_max <= 16 ? 16 : nd_max <= 32 ? 32 : nd_max <= 48 ? 48 : 64;
    K.nb = nb;
    if (nb == 64 && S.ld % 64 == 0 && S.ld >= 128) {
        // k_sweep_rl: strips of 64 W columns, pivot rows in registers, rows
        // and multipliers streamed into LDS; W = 4 waves, two batches in
        // flight, two workgroups per CU, row runs split by workgroup age
        // (plan_sweep_grid).  (Until late in round 6 runs of 16384+ rows -- cfg4 --
        // took one 8-wave, 4-deep workgroup per CU; with the split the 4-wave
        // pass is faster there too: cfg4 785-817 -> 759-779 us per launch on
        // two boxes, the 16384-row rank equal, profiles/r06/ab_r06_sweep_w4.txt).
        // Ranks sharing one GPU (tests and rehearsals: share > 1) with
        // 16384+ rows keep the 8-wave pass, one workgroup per CU: each rank's
        // XCD-shard selection is persistent and holds a wave on the CUs'
        // SIMDs while the other rank still sweeps, and the 4-wave pass's
        // 512 workgroups could then not all be placed (a co-located 2-GPU
        // rank pair timed out, tests/test_gpu_r4_procs.py)
        const bool w8 = S.share > 1 && S.rows >= 16384;
        K.rl = true;
        K.W = w8 ? 8 : 4;
        K.D = w8 ? 4 : 2;
        // out of place into the handle's other buffer when it has one (the
        // host then takes Tout as the tableau; see Args::dflips), with
        // non-temporal loads and stores (SA | 2): a tableau that large is far
        // beyond the Infinity Cache, and the pass then does not evict what the
        // selection keeps there -- cfg4 sweep 787-806 -> 775-781 us, selection
        // 7.12-7.15 -> 6.84-6.93 us per pivot (same box); at cfg3 (in place)
        // they cost the selection its cached tableau (4.50 -> 4.65 us)
        K.oop = S.second_buffer;
        // a group of nexp = 49..63 pivots: the pivot rows and multipliers
        // past it zeroed (stale rows of an earlier group otherwise; rows of
        // P and entries of MQ that no selection of this group writes), so
        // the pass treats them as exact no-ops
        K.nexp = nd_max < nb ? nd_max : nb;
    }
    return K;
}

inline SweepPlan plan_sweep_grid(const SweepShape &S, const SweepKernel &K, const SweepEnv &E)
{
    const int bpc = E.bpc;
    if (K.rl) {
        const int WL = K.W;
        // the columns swept: 0..n (the padding past them is 0 and stays 0).
        // Whole strips of 64 WL columns; a last partial strip of <= 64
        // columns is dealt out to every block (tail)
        const long long ncol = S.n + 1, nfull = ncol / (64 * WL), rest = ncol - nfull * 64 * WL;
        const bool spread = E.tail_mode != 0 && nfull >= 1 && rest > 0 && rest <= 64;
        const long long nsg = spread ? nfull : (ncol + 64 * WL - 1) / (64 * WL);
        const long long slots = (long long)E.cus * bpc;
        long long nrun = slots / nsg;
        if (nrun < 1) nrun = 1;
        long long run = (S.rows + nrun - 1) / nrun;
        run = (run + 7) / 8 * 8;                 // whole 8-row batches (the multipliers' quads)
        nrun = (S.rows + run - 1) / run;
        // Two workgroups per CU (the 4-wave pass): the grid's first half of
        // runs -- dispatched first, each CU's older workgroup, which the
        // CU's wave-age issue priority runs ahead -- takes SWEEP_SPLIT of the
        // rows, the second half the rest.  Equal runs ended bimodally (the
        // older workgroups at 66-78 us, the younger, then alone on the CU at
        // one wave per SIMD, at 93-102 us: profiles/r06/sweep_blocks_r06_cfg3.txt);
        // cfg3 sweep 104-106 -> 98-100 us (profiles/r06/ab_r06_sweep_split.txt).
        // LPGPU_SWEEP_SPLIT=f overrides (0: equal runs)
        long long runb = run;
        int na = (int)nrun;
        if (E.split > 0.0 && E.split < 1.0 && bpc == 2 && nrun >= 2 && nrun % 2 == 0) {
            const long long h = nrun / 2;
            long long ra = ((long long)(E.split * (double)S.rows) / h + 7) / 8 * 8;
            long long rb = ((S.rows - h * ra + h - 1) / h + 7) / 8 * 8;
            // (every run starts inside the tableau and the runs cover it)
            if (ra > 0 && rb > 0 && h * ra + h * rb >= S.rows && h * ra + (h - 1) * rb < S.rows) {
                run = ra;
                runb = rb;
                na = (int)h;
            }
        }
        const long long tail = spread ? ((S.rows + nrun * nsg - 1) / (nrun * nsg) + 7) / 8 * 8 : 0;
        return SweepPlan{K, nsg, nrun, run, runb, na, tail, nfull * 64 * WL, ncol, nrun * nsg};
    }
    // k_sweep_dp2 (in place), 10-wave workgroups on 128-column strips
    constexpr int RW = 4;
    const long long ns = (S.ld + 127) / 128;
    // the last strip (column n and the pitch's padding) spread over all
    // blocks where the runs are long (>= 2048 rows per block: the grid then
    // fills every resident slot); at short runs the extra piece (a P restage
    // + one batch) costs more than the slots give back
    const long long slots = (long long)E.cus * bpc;
    const bool tailed = ns >= 2 && (E.tail_mode == 2 || (E.tail_mode == 1 && S.rows * (ns - 1) >= 2048 * slots));
    const long long nsg = tailed ? ns - 1 : ns;   // strips with blocks of their own
    long long nrun = slots / nsg;
    if (nrun < 1) nrun = 1;
    long long run = (S.rows + nrun - 1) / nrun;
    run = (run + RW - 1) / RW * RW;
    nrun = (S.rows + run - 1) / run;
    // tail rows per block: a multiple of the batch (the multipliers' 4-row quads)
    const long long tail = tailed ? ((S.rows + nrun * nsg - 1) / (nrun * nsg) + RW - 1) / RW * RW : 0;
    return SweepPlan{K, nsg, nrun, run, run, (int)nrun, tail, 0, 0, nrun * nsg};
}

inline SweepPlan plan_sweep(const SweepShape &S, const SweepEnv &E)
{
    return plan_sweep_grid(S, choose_sweep_kernel(S), E);
}

// ---- the persistent selections ---------------------------------------------
// One compiled variant of a persistent selection kernel and the dynamic LDS
// its launch would ask for.
struct Variant {
    bool sel;        // k_sel<ipl, nb, xr, xs> (select.hip), else k_group<nr, ipl, rpl, xr, hk>
    int nr, ipl;
    int rpl;         // k_group: own rows per lane; k_sel: nb (32 / 64)
    bool xr, xs, hk;
    size_t lds;
};
// resident blocks per CU a launch of the variant may rely on (< 1: it cannot
// run), or OCC_MISSING: no such compiled variant.  On the device:
// persistent_occupancy (kernels.hip)
constexpr int OCC_MISSING = -(1 << 30);
using Occupancy = std::function<int(const Variant &)>;

// the one-XCD selection (select.hip): g <= 64 blocks, one own row per lane,
// the variable columns 1..n split evenly; g == 0 if the shape does not fit.
// xs_ok (single device): a tableau too tall for one XCD may run as XS_SHARDS
// row shards of <= 64 g rows, one per XCD, in one launch (geo.xs)
// share: ranks of a job on this GPU whose launches must be resident together
// (XR; the one-XCD kernel puts each on its own XCD, Args::xtarget, the XCD
// shards need share x g blocks on every XCD)
inline GroupGeom plan_sel(long long rc, long long n, int bmax, int xcd_cus, bool xr, bool xs_ok, int share,
                          const Occupancy &occ)
{
    GroupGeom G;
    if (rc < 1 || n < 1 || bmax < 1 || bmax > BMAX) return G;
    // one XCD, or (too tall for one: more than 64 x 64 rows) XS_SHARDS row
    // shards of rps rows, one per XCD, each shard's blocks over all columns
    int xs = 0;
    long long rps = rc;
    if ((rc + 63) / 64 > 64) {
        if (!xs_ok || bmax <= 32) return G;
        xs = XS_SHARDS;
        rps = (rc + XS_SHARDS - 1) / XS_SHARDS;
    }
    // the fewest blocks (g) with every lane at most 4 columns, or more where
    // a block's LDS (the pivot values of its columns) leaves too few blocks
    // per CU for g on one XCD
    const long long g0 = std::max((rps + 63) / 64, (n + 255) / 256);
    const int nb = bmax <= 32 ? 32 : 64;
    long long g = 0, cpb = 0;
    int ipl = 0, per_cu = 0;
    size_t lds = 0;
    bool bad = false;
    auto fits = [&](long long gc) {
        cpb = (n + gc - 1) / gc;
        ipl = (int)((cpb + 63) / 64);
        if (ipl == 3) ipl = 4;
        if (ipl > 4) return false;
        lds = ((size_t)cpb * (nb + 2) + 8) * sizeof(double);   // + the row chain's read-ahead slack
        per_cu = occ(Variant{true, 1, ipl, nb, xr, xs > 0, false, lds});
        if (per_cu == OCC_MISSING) {
            bad = true;
            return false;
        }
        // blocks this launch and the co-located ranks' need on one XCD at once.
        // XCD shards: every block works, share x gc per XCD.  One XCD (each
        // co-located rank on its own, Args::xtarget): gc, plus one free slot --
        // the other ranks' grids deal 7 of every 8 blocks to XCDs they do not
        // work on, and those idle blocks (exiting at once) still need a slot
        // to pass through in dispatch order: with the XCD full, the other
        // rank's launch stalls there and never reaches its own XCD
        const long long need = xs ? gc * std::max(share, 1) : share > 1 ? gc + 1 : gc;
        return per_cu >= 1 && need <= (long long)per_cu * xcd_cus;
    };
    // XCD shards: 64 blocks first where they fit -- the shard's rows are few
    // (2/4-GPU ranks of cfg4: 1024 / 2048 per XCD), the columns are what a
    // lane's chain walks, and two columns per lane beat four: 8192 x 8192
    // 102.9k -> 109.4k, 16384 x 8192 77.7k -> 80.9k pivots/s (round 5,
    // scripts/geo_probe.py xs)
    if (xs && g0 < 64 && fits(64)) g = 64;
    for (long long gc = g0; g == 0 && !bad && gc <= 64; gc = gc < 64 && gc + 8 > 64 ? 64 : gc + 8)
        if (fits(gc)) g = gc;
    if (g == 0) return G;
    G.g = g;
    G.nr = 1;
    G.ipl = ipl;
    G.rpl = 1;
    G.xmode = 1;
    G.sel = nb;
    G.xs = xs;
    G.lds = lds;
    G.per_cu = per_cu;
    return G;
}

// k_group, or k_sel where the shape fits it: see group_geom (engine.h).
// cus: the device's compute units; hier: LPGPU_HIER
inline GroupGeom plan_group(long long rc, long long ld, long long n, int bmax, int xr, int nshard, int share,
                            bool xs_ok, int cus, int hier, const Occupancy &occ)
{
    GroupGeom G;
    if (rc < 1 || ld < 1 || ld >= 0x7fffffffLL || rc >= 0x7fffffffLL || bmax < 1 || bmax > BMAX ||
        nshard < 1 || share < 1)
        return G;   // indices travel as 31 bits
    const int xcd_cus = cus / 8;
    // the one-XCD selection k_sel (select.hip) where the shape fits it
    // (ranks sharing a GPU: only the XR variant that may use one XCD, which
    // then sizes for the co-located ranks itself)
    if (xr != 1 && nshard == 1 && (share == 1 || xr == 2)) {
        const GroupGeom S = plan_sel(rc, n, bmax, xcd_cus, xr != 0, xs_ok && xr != 1, share, occ);
        if (S.g > 0) return S;
    }
    // candidate block counts, preferred first: at least one own row per
    // lane-slot, every lane at most 4 columns; with a few extra blocks every
    // lane down to 2 columns ("wide"), or not ("narrow", fewer blocks: fits
    // where the wide one does not); more blocks where one's LDS would exceed
    // GROUP_LDS_MAX
    struct Cand {
        long long g;
        int rpl;
    };
    Cand cand[2 * GROUP_MAXRPL];
    int nc = 0;
    for (int rpl = 1; rpl <= GROUP_MAXRPL; rpl *= 2)   // compiled: 1, 2, 4 rows per lane
        for (int wide = 1; wide >= 0; --wide) {
            long long g = (rc + 64LL * rpl - 1) / (64LL * rpl);
            if (g < GROUP_MINBLOCKS) g = GROUP_MINBLOCKS;
            const long long g2 = (ld + 2 * GROUP_THREADS - 1) / (2 * GROUP_THREADS);
            const long long g4 = (ld + 4 * GROUP_THREADS - 1) / (4 * GROUP_THREADS);
            if (wide && g2 > g && g2 <= g + g / 8) g = g2;
            if (g4 > g) g = g4;
            while (g < GROUP_MAXBLOCKS && group_lds(rc, ld, g, bmax) > GROUP_LDS_MAX) g *= 2;
            if (g > GROUP_MAXBLOCKS) g = GROUP_MAXBLOCKS;
            bool dup = false;
            for (int k = 0; k < nc; ++k) dup = dup || (cand[k].g == g && cand[k].rpl == rpl);
            if (!dup) cand[nc++] = Cand{g, rpl};
        }
    // every block of every launch that waits on this one must be resident at
    // the same time.  Workgroups are dealt round-robin over the 8 XCDs, so
    // each XCD must hold its eighth: one XCD (L2-resident hand-offs, xmode)
    // where the blocks fit there, else the whole device
    // blocks spread over the XCDs: a multiple of 8 of them, so that k_group's
    // two-level exchange applies (G / 8 blocks per XCD; LPGPU_HIER=0: flat)
    for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < nc; ++k) {
            long long g = cand[k].g;
            if (pass == 1 && hier && !xr && nshard == 1 && g >= 64)
                g = std::min<long long>((g + 7) / 8 * 8, GROUP_MAXBLOCKS);
            const int rpl = cand[k].rpl;
            const long long cpb = (ld + g - 1) / g, rpb = (rc + g - 1) / g;
            const long long lds = group_lds(rc, ld, g, bmax);
            if (cpb > 4 * GROUP_THREADS || rpb > (long long)rpl * GROUP_THREADS || lds > GROUP_LDS_MAX)
                continue;
            int nr = (int)((g + GROUP_THREADS - 1) / GROUP_THREADS);
            nr = nr <= 1 ? 1 : nr <= 2 ? 2 : 4;
            int ipl = (int)((cpb + GROUP_THREADS - 1) / GROUP_THREADS);
            ipl = ipl <= 2 ? 2 : (ipl == 3 && nr <= 2) ? 3 : 4;
            if (rpl >= 2) {
                nr = 4;
                ipl = ipl <= 2 ? 2 : 4;
            }
            // spread single-device groups: the variant with the two-level exchange
            const bool hk = pass == 1 && hier && !xr && nshard == 1 && g % 8 == 0 && g >= 64;
            const int per_cu = occ(Variant{false, nr, ipl, rpl, xr != 0, false, hk, (size_t)lds});
            if (per_cu < 1) continue;   // (OCC_MISSING too)
            const bool one = pass == 0;
            if (one && !(xr != 1 && nshard == 1 && share == 1 && g <= (long long)per_cu * xcd_cus))
                continue;
            // ranks sharing a GPU launch their groups unsynchronised, so another
            // rank's sweep or set-up kernel can hold a slot while this group must
            // be resident: there, one block slot per CU stays free (4 ranks of
            // cfg4 on one GPU filled 2 of 2 slots per CU and timed out, round 2)
            const int per_cu_job = share > 1 ? per_cu - 1 : per_cu;
            if (!one && (g * nshard * share + 7) / 8 > (long long)per_cu_job * xcd_cus) continue;
            G.g = g;
            G.nr = nr;
            G.ipl = ipl;
            G.rpl = rpl;
            G.lds = (size_t)lds;
            G.per_cu = per_cu;
            G.xmode = one ? 1 : 0;
            G.hk = hk ? 1 : 0;
            return G;
        }
    return GroupGeom{};
}

}  // namespace lpk
