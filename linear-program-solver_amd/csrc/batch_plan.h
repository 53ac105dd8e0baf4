// Launch planning of a ragged batch (lp_ragged_*): which LPs of a
// batch of mixed shapes share a launch.  Pure host code in the style of
// geometry.h -- no HIP, no environment; what the runtime knows (how many workgroups
// of an instantiation a CU holds by wave slots and registers) arrives as
// arguments -- so csrc/batch_plan_check.cpp runs it under the host sanitizers
// (tests/test_ragged_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace lpk {

constexpr int64_t PLAN_LDS_MAX = 160 * 1024;        // one CU's LDS
constexpr int64_t PLAN_NO_FIT = INT64_MAX;          // a shape no formula below is evaluated for

// lp_batch_create's formula: (m+1) rows at the odd pitch (n+1) | 1, the
// normalised pivot row, the multipliers and 16 doubles of reduction scratch
inline int64_t plan_plain_pitch(int64_t n) { return (n + 1) | 1; }
inline int64_t plan_plain_lds(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_NO_FIT;
    const int64_t pitch = plan_plain_pitch(n);
    return ((m + 1) * pitch + pitch + (m + 1) + 16) * 8;
}

// lp_twophase_lds_bytes: the same at the widened pitch (n+1+m) | 1, plus the
// basis (m int32)
inline int64_t plan_twophase_pitch(int64_t m, int64_t n) { return (n + 1 + m) | 1; }
inline int64_t plan_twophase_lds(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_NO_FIT;
    const int64_t pitch = plan_twophase_pitch(m, n);
    return ((m + 1) * pitch + pitch + (m + 1) + 16 + (m + 1) / 2) * 8;
}

// one wave per LP up to one_wave_elems live elements, four above; the
// two-phase count is taken on the widest artificial problem
inline int plan_plain_waves(int64_t m, int64_t n, int64_t one_wave_elems)
{
    return (m + 1) * (n + 1) <= one_wave_elems ? 1 : 4;
}
inline int plan_twophase_waves(int64_t m, int64_t n, int64_t one_wave_elems)
{
    return (m + 1) * (n + 1 + m) <= one_wave_elems ? 1 : 4;
}

inline int64_t plan_need(bool twophase, int64_t m, int64_t n)
{
    return twophase ? plan_twophase_lds(m, n) : plan_plain_lds(m, n);
}
inline int plan_waves(bool twophase, int64_t m, int64_t n, int64_t one_wave_elems)
{
    return twophase ? plan_twophase_waves(m, n, one_wave_elems) : plan_plain_waves(m, n, one_wave_elems);
}

// one launch: `order` lists its LPs ascending, lds is the largest need among
// them, lps_per_cu what a CU then holds of them (slots, registers and LDS)
struct PlanBin {
    int waves = 1;
    int lps_per_cu = 0;
    int64_t lds = 0;
    std::vector<int32_t> order;
    bool device = false;            // the bin of the device-placed LPs (plan_placed)
};

struct BatchPlan {
    std::vector<PlanBin> bins;      // in launch order: largest LDS first
    int64_t too_large = -1;         // first LP whose need exceeds a CU's LDS (then no bins)
};

// LP i goes to the bin keyed (waves_i, min(slot_cap[waves_i], 160 KiB / need_i)).
// All members of a bin hold the same number k of LPs per CU by LDS (or at
// least slot_cap of them), so does the largest, and launching every member at
// the largest need still fits k: no LP runs at fewer LPs per CU than a uniform
// batch of its own shape would.  The second key component lies in
// 1..slot_cap[waves], hence at most slot_cap1 + slot_cap4 bins.
inline BatchPlan plan_ragged(int64_t count, const int64_t *m, const int64_t *n, bool twophase, int slot_cap1,
                             int slot_cap4, int64_t one_wave_elems)
{
    BatchPlan P;
    std::map<std::pair<int, int>, PlanBin> bins;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t need = plan_need(twophase, m[i], n[i]);
        if (need > PLAN_LDS_MAX) {
            P.too_large = i;
            return P;
        }
        const int waves = plan_waves(twophase, m[i], n[i], one_wave_elems);
        const int cap = std::max(1, waves == 1 ? slot_cap1 : slot_cap4);
        const int k = (int)std::min<int64_t>(cap, PLAN_LDS_MAX / need);
        PlanBin &b = bins[{waves, k}];
        b.waves = waves;
        b.lps_per_cu = k;
        b.lds = std::max(b.lds, need);
        b.order.push_back((int32_t)i);      // i ascends
    }
    for (auto &kv : bins) P.bins.push_back(std::move(kv.second));
    std::stable_sort(P.bins.begin(), P.bins.end(), [](const PlanBin &a, const PlanBin &b) {
        return a.lds != b.lds ? a.lds > b.lds : a.waves > b.waves;
    });
    return P;
}

// ---------------------------------------------------------------------------
// Placement (lp_placed_create / lp_placed_create_ragged):
// an LP's tableau lives in a CU's LDS for the life of a launch, or stays in
// device memory with only the side buffers in LDS.  The values are
// LP_PLACE_* of include/lpgpu.h.
// ---------------------------------------------------------------------------
constexpr int PLAN_PLACE_LDS = 0, PLAN_PLACE_AUTO = 1, PLAN_PLACE_DEVICE = 2;
constexpr int PLAN_PLACE_BAD = -1;          // an unknown request
constexpr int PLAN_PLACE_TOO_LARGE = -2;    // no placement the request allows takes the LP

// LDS of a device-placed LP (lp_placed_lds_bytes): the normalised pivot
// row (n+1), the multipliers (m+1) and 16 doubles of reduction scratch
inline int64_t plan_device_lds(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_NO_FIT;
    return ((n + 1) + (m + 1) + 16) * 8;
}

// where LP (m, n) goes under `place`: PLAN_PLACE_LDS or PLAN_PLACE_DEVICE, or
// one of the two refusals.  AUTO prefers LDS whenever the LP fits it.
inline int plan_place(int place, int64_t m, int64_t n)
{
    if (place != PLAN_PLACE_LDS && place != PLAN_PLACE_AUTO && place != PLAN_PLACE_DEVICE) return PLAN_PLACE_BAD;
    if (place != PLAN_PLACE_DEVICE && plan_plain_lds(m, n) <= PLAN_LDS_MAX) return PLAN_PLACE_LDS;
    if (place == PLAN_PLACE_LDS) return PLAN_PLACE_TOO_LARGE;
    return plan_device_lds(m, n) <= PLAN_LDS_MAX ? PLAN_PLACE_DEVICE : PLAN_PLACE_TOO_LARGE;
}

// pivots one launch may run on a device-placed LP: `chunk`, capped so that a
// launch applies at most `work` element updates per LP; at least 1
inline int64_t plan_device_chunk(int64_t chunk, int64_t work, int64_t m, int64_t n)
{
    return std::max<int64_t>(1, std::min(chunk, work / ((m + 1) * (n + 1))));
}

// What plan_placed and plan_phased share: the LPs that `where_of` sends to
// device memory are one bin, ascending, launched first (they run longest) at
// dev_waves waves per LP and the largest `dev_need` among them; dev_slot_cap is
// what a CU holds of that kernel by wave slots and registers.  The LDS-placed
// LPs are binned by plan_ragged as a batch of their own would be, their
// indices mapped back.
template <class Where, class Need>
inline BatchPlan plan_split(int64_t count, const int64_t *m, const int64_t *n, bool twophase, Where where_of,
                            Need dev_need, int slot_cap1, int slot_cap4, int64_t one_wave_elems, int dev_waves,
                            int dev_slot_cap)
{
    BatchPlan P;
    PlanBin dev;
    dev.device = true;
    dev.waves = dev_waves;
    std::vector<int32_t> at;                // the LDS-placed LPs, ascending
    std::vector<int64_t> lm, ln;
    for (int64_t i = 0; i < count; ++i) {
        const int where = where_of(m[i], n[i]);
        if (where < 0) {
            P.too_large = i;
            return P;
        }
        if (where == PLAN_PLACE_DEVICE) {
            dev.lds = std::max(dev.lds, dev_need(m[i], n[i]));
            dev.order.push_back((int32_t)i);
        } else {
            at.push_back((int32_t)i);
            lm.push_back(m[i]);
            ln.push_back(n[i]);
        }
    }
    if (!dev.order.empty()) {
        dev.lps_per_cu = (int)std::min<int64_t>(std::max(1, dev_slot_cap), PLAN_LDS_MAX / dev.lds);
        P.bins.push_back(std::move(dev));
    }
    BatchPlan L =
        plan_ragged((int64_t)at.size(), lm.data(), ln.data(), twophase, slot_cap1, slot_cap4, one_wave_elems);
    for (PlanBin &b : L.bins) {
        for (int32_t &i : b.order) i = at[(size_t)i];
        P.bins.push_back(std::move(b));
    }
    return P;
}

// The plan of the plain call on a placed batch: plan_split by plan_place and
// plan_device_lds.
inline BatchPlan plan_placed(int64_t count, const int64_t *m, const int64_t *n, int place, int slot_cap1,
                             int slot_cap4, int64_t one_wave_elems, int dev_waves, int dev_slot_cap)
{
    return plan_split(
        count, m, n, false, [place](int64_t mi, int64_t ni) { return plan_place(place, mi, ni); }, plan_device_lds,
        slot_cap1, slot_cap4, one_wave_elems, dev_waves, dev_slot_cap);
}

// ---------------------------------------------------------------------------
// Phased batches (lp_phased_*): the two-phase call on a placed
// batch.  An LP whose widened tableau does not fit a CU's LDS runs phase 1
// and phase 2 from device memory (k_twophase_dev).
// ---------------------------------------------------------------------------

// LDS of a device-placed two-phase LP (lp_phased_lds_bytes): the normalised
// pivot row at the widest live width (n+1+m), the multipliers (m+1), 16
// doubles of reduction scratch and the basis (m int32) as k_twophase keeps it
inline int64_t plan_phased_lds(int64_t m, int64_t n)
{
    if (m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_NO_FIT;
    return ((n + 1 + m) + (m + 1) + 16 + (m + 1) / 2) * 8;
}

// plan_place for the two-phase call: the LDS test is plan_twophase_lds, so an
// LP can be LDS-placed for the plain call and device-placed for this one
inline int plan_place_phased(int place, int64_t m, int64_t n)
{
    if (place != PLAN_PLACE_LDS && place != PLAN_PLACE_AUTO && place != PLAN_PLACE_DEVICE) return PLAN_PLACE_BAD;
    if (place != PLAN_PLACE_DEVICE && plan_twophase_lds(m, n) <= PLAN_LDS_MAX) return PLAN_PLACE_LDS;
    if (place == PLAN_PLACE_LDS) return PLAN_PLACE_TOO_LARGE;
    return plan_phased_lds(m, n) <= PLAN_LDS_MAX ? PLAN_PLACE_DEVICE : PLAN_PLACE_TOO_LARGE;
}

// plan_device_chunk taken on the widened element count (m+1)(n+1+m): drive-out
// pivots count as pivots
inline int64_t plan_phased_chunk(int64_t chunk, int64_t work, int64_t m, int64_t n)
{
    return std::max<int64_t>(1, std::min(chunk, work / ((m + 1) * (n + 1 + m))));
}

// The plan of the two-phase call on a placed batch: plan_split by
// plan_place_phased and plan_phased_lds, the LDS-placed LPs through
// plan_ragged(twophase).
inline BatchPlan plan_phased(int64_t count, const int64_t *m, const int64_t *n, int place, int slot_cap1,
                             int slot_cap4, int64_t one_wave_elems, int dev_waves, int dev_slot_cap)
{
    return plan_split(
        count, m, n, true, [place](int64_t mi, int64_t ni) { return plan_place_phased(place, mi, ni); },
        plan_phased_lds, slot_cap1, slot_cap4, one_wave_elems, dev_waves, dev_slot_cap);
}

// ---------------------------------------------------------------------------
// Teamed batches (lp_teamed_*): a device-placed LP worked on by
// a team of G workgroups, one launch per pivot (k_batch_team).  Each workgroup
// of a team selects the pivot itself and updates one contiguous range of the
// LP's E = (m+1)(n+1) elements.
// ---------------------------------------------------------------------------
constexpr int PLAN_TEAM_REFUSED = -1;       // a request no LP of this shape can take

// The team of LP (m, n).  request 1: one workgroup, the placed path.  request
// G > 1: G, refused above team_max or above E / 2 (a range holds at least one
// pair).  request 0 (auto): as many workgroups as the chip has room for when
// n_device_lps LPs share `slots` resident workgroups (CUs times the workgroups
// of k_batch_team a CU holds), but no range below team_min_elems elements; and
// no team at all where n_device_lps > E / team_lp_elems, the measured limit
// (DESIGN.md 4l): what a team saves per pivot grows with E, what one launch per
// pivot costs grows with the LPs in it.  team_lp_elems <= 0: no such limit.
inline int plan_team_size(int request, int64_t n_device_lps, int64_t m, int64_t n, int64_t slots, int team_max,
                          int64_t team_min_elems, int64_t team_lp_elems = 0)
{
    if (request < 0 || m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_TEAM_REFUSED;
    if (request == 1) return 1;
    const int64_t E = (m + 1) * (n + 1);
    if (request > 1) return request > team_max || request > E / 2 ? PLAN_TEAM_REFUSED : request;
    const int64_t lps = std::max<int64_t>(1, n_device_lps);
    const int64_t room = slots / lps;
    const int64_t by_size = E / std::max<int64_t>(2, team_min_elems);
    if (team_lp_elems > 0 && lps > E / team_lp_elems) return 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(room, by_size), std::max(1, team_max)));
}

// The G ranges of a team: range r is [e[r], e[r+1]) of [0, E), in order, none
// empty, for 1 <= G <= max(1, E / 2).  The LP starts at double `toff` of its
// buffer and is cut into the aligned pairs of that buffer (a pair begins where
// toff + e is even; the first and the last pair may hold one element of the LP);
// every interior end is a pair boundary, and a range holds floor(NP / G) or
// ceil(NP / G) of the NP pairs, so sizes differ by at most one pair.
inline std::vector<int64_t> plan_team_ranges(int64_t E, int64_t toff, int G)
{
    const int64_t first = toff / 2, last = (toff + E - 1) / 2, NP = last - first + 1;
    std::vector<int64_t> e((size_t)G + 1);
    for (int r = 0; r <= G; ++r) {
        const int64_t at = 2 * (first + r * NP / G) - toff;     // -1 or 0 at r = 0, E or E + 1 at r = G
        e[(size_t)r] = std::min(E, std::max<int64_t>(0, at));
    }
    return e;
}

// one workgroup of a teamed launch: rank `rank` of the G of LP `lp` updates
// elements [e0, e1) of it
struct TeamWG {
    int32_t lp, rank, G, e0, e1;
};

// The workgroup table of a batch: the LPs with a team above 1, ascending, each
// with its ranks in order.  team[i] <= 1: LP i is not teamed.
inline std::vector<TeamWG> plan_team_table(int64_t count, const int64_t *m, const int64_t *n, const int64_t *toff,
                                           const int32_t *team)
{
    std::vector<TeamWG> wg;
    for (int64_t i = 0; i < count; ++i) {
        if (team[i] <= 1) continue;
        const std::vector<int64_t> e = plan_team_ranges((m[i] + 1) * (n[i] + 1), toff[i], team[i]);
        for (int r = 0; r < team[i]; ++r)
            wg.push_back(TeamWG{(int32_t)i, r, team[i], (int32_t)e[(size_t)r], (int32_t)e[(size_t)r + 1]});
    }
    return wg;
}

// ---------------------------------------------------------------------------
// Solution batches (lp_solution_canonical / lp_solution_gather):
// small kernels over the flat packed stack.  A lane is one tableau column of
// one LP of the window (column 0, the b column, included), adjacent lanes on
// adjacent columns, so a row read of a wave is one contiguous run; or one
// basis entry of one LP.
// ---------------------------------------------------------------------------
#ifdef __HIP__
#define LPK_PLAN_HD __host__ __device__
#else
#define LPK_PLAN_HD
#endif

constexpr int PLAN_SCAN_COLS = 64;          // columns per workgroup of the scan: one wave wide
constexpr int PLAN_SCAN_MAX_SLICES = 16;    // row slices (waves) per workgroup at the most
constexpr int PLAN_FLAT_THREADS = 256;      // the flat kernels' workgroup

// Row slices of the canonical scan: wave s of a workgroup reads constraint
// rows s, s + S, ... of its 64 columns, and the S partial results meet in LDS.
// One wave while a column is short (no LDS, no barrier: the 9 x 11 end), more
// as the tallest LP of the window grows (the one-LP 513 x 513 end).
inline int plan_scan_slices(int64_t max_m)
{
    return max_m <= 16 ? 1 : max_m <= 128 ? 4 : PLAN_SCAN_MAX_SLICES;
}

// a launch over `lanes` lanes, `per_block` of them per workgroup of `threads`
// threads; blocks < 0: more than a grid holds
struct FlatGrid {
    int64_t lanes = 0, blocks = 0;
    int threads = 0, slices = 1;
};
inline FlatGrid plan_flat_grid(int64_t lanes, int per_block, int threads)
{
    FlatGrid g;
    g.lanes = lanes;
    g.threads = threads;
    g.blocks = lanes <= 0 ? 0 : (lanes + per_block - 1) / per_block;
    if (g.blocks > INT32_MAX) g.blocks = -1;
    return g;
}
// the scan: cols = the tableau columns of the window, max_m its tallest LP
inline FlatGrid plan_scan_grid(int64_t cols, int64_t max_m)
{
    const int S = plan_scan_slices(max_m);
    FlatGrid g = plan_flat_grid(cols, PLAN_SCAN_COLS, PLAN_SCAN_COLS * S);
    g.slices = S;
    return g;
}

// The LP of lane g: the last i of [lo, hi) with start(i) <= g, where start
// ascends strictly from start(lo) <= g.  At most 64 halvings of hi - lo.
template <class Start>
LPK_PLAN_HD inline long long plan_lane_lp(long long lo, long long hi, long long g, Start start)
{
    for (int it = 0; it < 64 && hi - lo > 1; ++it) {
        const long long mid = lo + (hi - lo) / 2;
        if (start(mid) <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// Problem-form batches (lp_problem_*): an LP arrives as the
// first ns + 1 columns of its tableau plus one sense per constraint row, and
// k_assemble writes the (m+1) x (n+1) tableau, n = ns + k, k the rows that are
// not equalities.  The t-th such row owns variable column ns + t.
// ---------------------------------------------------------------------------
constexpr int PLAN_SENSE_LE = 0, PLAN_SENSE_GE = 1, PLAN_SENSE_EQ = 2;   // LP_SENSE_* of include/lpgpu.h
constexpr int64_t PLAN_PROBLEM_BAD_SENSE = -1;  // a sense outside 0..2 (*bad_row names the first)
constexpr int64_t PLAN_PROBLEM_NO_VARS = -2;    // k >= n: no structural variable would be left
constexpr int64_t PLAN_PROBLEM_BAD_SHAPE = -3;  // NULL senses, m or n <= 0

// The slack table of one LP: out[r] = +(1 + j) where row r is <= and owns
// variable column j (tableau column 1 + j), -(1 + j) where it is >=, 0 for an
// equality.  Returns ns = n - k, or one of the refusals above with `out`
// untouched.  out may be NULL (the count alone).
inline int64_t plan_problem_slack(const int8_t *sense, int64_t m, int64_t n, int32_t *out, int64_t *bad_row = nullptr)
{
    if (!sense || m <= 0 || n <= 0 || m >= (1 << 20) || n >= (1 << 20)) return PLAN_PROBLEM_BAD_SHAPE;
    int64_t k = 0;
    for (int64_t r = 0; r < m; ++r) {
        if (sense[r] < PLAN_SENSE_LE || sense[r] > PLAN_SENSE_EQ) {
            if (bad_row) *bad_row = r;
            return PLAN_PROBLEM_BAD_SENSE;
        }
        k += sense[r] != PLAN_SENSE_EQ ? 1 : 0;
    }
    if (k >= n) return PLAN_PROBLEM_NO_VARS;
    const int64_t ns = n - k;
    if (out)
        for (int64_t r = 0, t = 0; r < m; ++r) {
            if (sense[r] == PLAN_SENSE_EQ) out[r] = 0;
            else out[r] = (int32_t)(sense[r] == PLAN_SENSE_LE ? 1 + ns + t : -(1 + ns + t)), ++t;
        }
    return ns;
}

// consecutive destination elements one lane of k_assemble writes: it finds its
// LP once and walks on (picked by measurement; the A/B builds
// move it with -DLPK_ASSEMBLE_RUN=)
#ifndef LPK_ASSEMBLE_RUN
#define LPK_ASSEMBLE_RUN 1
#endif
constexpr int PLAN_ASSEMBLE_RUN = LPK_ASSEMBLE_RUN;
static_assert(PLAN_ASSEMBLE_RUN >= 1 && PLAN_ASSEMBLE_RUN <= 16, "elements per lane of k_assemble");

// the launch of k_assemble over `elems` destination elements
inline FlatGrid plan_assemble_grid(int64_t elems)
{
    const int64_t lanes = elems <= 0 ? 0 : (elems + PLAN_ASSEMBLE_RUN - 1) / PLAN_ASSEMBLE_RUN;
    return plan_flat_grid(lanes, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS);
}

// a destination element's place: LP, tableau row and column
struct ProblemAt {
    long long lp;
    int row, col;
};
// element `rem` of an LP whose tableau is w = n + 1 doubles wide
LPK_PLAN_HD inline ProblemAt plan_problem_at(long long lp, long long rem, int w)
{
    ProblemAt at;
    at.lp = lp;
    at.row = (int)(rem / w);
    at.col = (int)(rem - (long long)at.row * w);
    return at;
}
// the element after `at` in an (m+1) x (n+1) LP; true where it is the next LP's first
LPK_PLAN_HD inline bool plan_problem_next(ProblemAt &at, int m, int n)
{
    if (++at.col <= n) return false;
    at.col = 0;
    if (++at.row <= m) return false;
    at.row = 0;
    ++at.lp;
    return true;
}

// what cell (row, col) of an assembled tableau holds: the staged value at
// P[row][col], +1.0, -1.0 or +0.0; slack_of_row is the row's table entry (0 for
// row 0).  col > ns >= 1, so a slack column is never 0.
constexpr int PLAN_CELL_ZERO = 0, PLAN_CELL_PLUS = 1, PLAN_CELL_MINUS = 2, PLAN_CELL_STAGED = 3;
LPK_PLAN_HD inline int plan_problem_cell(int col, int ns, int slack_of_row)
{
    if (col <= ns) return PLAN_CELL_STAGED;
    return slack_of_row == col ? PLAN_CELL_PLUS : slack_of_row == -col ? PLAN_CELL_MINUS : PLAN_CELL_ZERO;
}

// One lane of k_assemble, on the host and on the device: the PLAN_ASSEMBLE_RUN
// elements from `e0` of a window of `elems` destination elements.  locate(e) is
// the LP of element e, shape(i) LP i's ProblemLp, slack(at) an entry of the
// slack table; put(dst, kind, src) stores one cell, a PLAN_CELL_* kind, dst and
// src indexing the window's tableaux and its staged problem blocks (src is
// read for PLAN_CELL_STAGED only).
struct ProblemLp {
    long long toff, poff;       // the LP's tableau and problem block, doubles from the window's first
    long long soff;             // its first row's entry in the slack table
    int m, n, ns;
};
template <class Locate, class Shape, class Slack, class Put>
LPK_PLAN_HD inline void plan_assemble_lane(long long e0, long long elems, Locate locate, Shape shape, Slack slack,
                                           Put put)
{
    if (e0 >= elems) return;
    const long long lp0 = locate(e0);
    ProblemLp L = shape(lp0);
    ProblemAt at = plan_problem_at(lp0, e0 - L.toff, L.n + 1);
    for (int r = 0; r < PLAN_ASSEMBLE_RUN; ++r) {
        const long long e = e0 + r;
        if (e >= elems) return;
        const int s = at.col > L.ns && at.row > 0 ? slack(L.soff + at.row - 1) : 0;
        put(e, plan_problem_cell(at.col, L.ns, s), L.poff + (long long)at.row * (L.ns + 1) + at.col);
        if (plan_problem_next(at, L.m, L.n) && e + 1 < elems) L = shape(at.lp);
    }
}

// ---------------------------------------------------------------------------
// Warm re-solves (lp_resolve_set_rhs): new right-hand sides on
// the stored tableaux.  A stored tableau is M . [the assembled one] for an
// invertible M, and the column a row's slack or surplus variable owns holds
// M's column of that row up to the sign s = +1 (<=) or -1 (>=), so the new
// column 0 is M . rhs, one short dot product per tableau row.  A lane of k_rhs
// is one (LP, row) pair of the window, rows 0..m_i, LP after LP: lane g of LP
// i's m_i + 1 starts at (boff(i) - boff(first)) + (i - first), which is also
// where the LP's m_i + 1 doubles begin in the packed rhs.
// ---------------------------------------------------------------------------

// the launch of k_rhs over the window's `pairs` = rows + LPs lanes
inline FlatGrid plan_rhs_grid(int64_t pairs) { return plan_flat_grid(pairs, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS); }

// lane g's place: the LP, its tableau row and where the LP's rhs begins
struct RhsAt {
    long long lp, base;
    int row;
};
// uniform batch: every LP has m + 1 lanes
LPK_PLAN_HD inline RhsAt plan_rhs_at(long long first, long long g, int m)
{
    const long long k = g / (m + 1);
    return RhsAt{first + k, k * (m + 1), (int)(g - k * (m + 1))};
}
// ragged batch: start(i) is the lane LP i begins at, ascending from start(first) = 0
template <class Start>
LPK_PLAN_HD inline RhsAt plan_rhs_at(long long first, long long hi, long long g, Start start)
{
    const long long lp = plan_lane_lp(first, hi, g, start);
    const long long base = start(lp);
    return RhsAt{lp, base, (int)(g - base)};
}

// one product and one sum of the loop below, each rounded to nearest on its
// own: never an fma (the host build is compiled with -ffp-contract=off)
LPK_PLAN_HD inline double plan_rhs_madd(double acc, double t, double b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(acc, __dmul_rn(t, b));
#else
    const double p = t * b;
    return acc + p;
#endif
}

// The new T[i][0] of tableau row i of an LP with m rows: slack(k) is row k's
// table entry +-(1 + j) (never 0: an LP with an equality is refused), cell(c)
// the stored T[i][c], c >= 1, and rhs(k) the LP's k-th new value, rhs(0) the
// stored _z cell.  The product with s is a flip of the sign bit.
template <class Slack, class Cell, class Rhs>
LPK_PLAN_HD inline double plan_rhs_cell(int i, int m, Slack slack, Cell cell, Rhs rhs)
{
    double acc = i == 0 ? rhs(0) : 0.0;
    for (int k = 0; k < m; ++k) {
        const int s = slack(k);
        const double t = cell(s > 0 ? s : -s);
        acc = plan_rhs_madd(acc, s > 0 ? t : -t, rhs(1 + k));
    }
    return acc;
}

// ---------------------------------------------------------------------------
// General-form batches (lp_general_*): min or max of c0 + c.x
// under A x {<=, >=, ==} b with one kind per variable -- x >= 0, x >= lb,
// lb <= x <= ub, x <= ub or free.  The standard form the solve kernels get has
// m' = m + nb rows and n' = ns + nf + k + nb columns: the ns variables, the
// negative parts of the nf FREE ones, then one slack per row that is not an
// equality, the nb bound rows (all <=, in variable order) after the m rows.
// ---------------------------------------------------------------------------
constexpr int PLAN_VAR_PLAIN = 0, PLAN_VAR_LOWER = 1, PLAN_VAR_BOXED = 2, PLAN_VAR_UPPER = 3,
              PLAN_VAR_FREE = 4;                 // LP_VAR_* of include/lpgpu.h
constexpr int64_t PLAN_GENERAL_BAD_SENSE = -1;   // a sense outside 0..2 (*bad names the first)
constexpr int64_t PLAN_GENERAL_BAD_KIND = -2;    // a kind outside 0..4 (*bad names the first)
constexpr int64_t PLAN_GENERAL_BAD_SHAPE = -3;   // NULL senses or kinds, m or ns <= 0 or too large

struct GeneralCounts {
    int64_t m = 0, ns = 0, nf = 0, nb = 0, k = 0;
    int64_t rows = 0, cols = 0;     // m' and n'
};

// the counts of one LP; 0, or one of the refusals above with `out` untouched
inline int64_t plan_general_counts(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns, GeneralCounts *out,
                                   int64_t *bad = nullptr)
{
    if (!sense || !kind || m <= 0 || ns <= 0 || m >= (1 << 19) || ns >= (1 << 18)) return PLAN_GENERAL_BAD_SHAPE;
    GeneralCounts c;
    c.m = m;
    c.ns = ns;
    for (int64_t r = 0; r < m; ++r) {
        if (sense[r] < PLAN_SENSE_LE || sense[r] > PLAN_SENSE_EQ) {
            if (bad) *bad = r;
            return PLAN_GENERAL_BAD_SENSE;
        }
        c.k += sense[r] != PLAN_SENSE_EQ ? 1 : 0;
    }
    for (int64_t j = 0; j < ns; ++j) {
        if (kind[j] < PLAN_VAR_PLAIN || kind[j] > PLAN_VAR_FREE) {
            if (bad) *bad = j;
            return PLAN_GENERAL_BAD_KIND;
        }
        c.nf += kind[j] == PLAN_VAR_FREE ? 1 : 0;
        c.nb += kind[j] == PLAN_VAR_BOXED ? 1 : 0;
    }
    c.rows = m + c.nb;
    c.cols = ns + c.nf + c.k + c.nb;
    if (out) *out = c;
    return 0;
}

// One entry per tableau column 1..ns+nf (index column - 1).  src = 2 j + f: the
// column holds variable j of the caller's block, its constraint rows with the
// sign bit flipped iff f (an UPPER variable, or the negative part of a FREE
// one), its cost flipped iff (maximise XOR f).  For the ns variables' own
// columns: brow the tableau row of a BOXED variable's bound row, neg the
// tableau column of a FREE variable's negative part, else 0; kind the LP_VAR_*.
struct GVar {
    int32_t src, brow, neg, kind;
};

// The tables of one LP: var[ns + nf], slack[m'] (plan_problem_slack over the
// senses extended by nb "<="), bvar[m'] (the variable of a bound row, -1 on the
// m rows).  Returns 0 or a refusal of plan_general_counts, nothing written.
inline int64_t plan_general_tables(const int8_t *sense, const int8_t *kind, int64_t m, int64_t ns, GVar *var,
                                   int32_t *slack, int32_t *bvar, int64_t *bad = nullptr)
{
    GeneralCounts c;
    const int64_t st = plan_general_counts(sense, kind, m, ns, &c, bad);
    if (st != 0) return st;
    std::vector<int8_t> ext(sense, sense + m);
    ext.resize((size_t)c.rows, (int8_t)PLAN_SENSE_LE);
    if (plan_problem_slack(ext.data(), c.rows, c.cols, slack) != ns + c.nf) return PLAN_GENERAL_BAD_SHAPE;
    for (int64_t r = 0; r < m; ++r) bvar[r] = -1;
    int64_t f = 0, t = 0;
    for (int64_t j = 0; j < ns; ++j) {
        GVar v{(int32_t)(2 * j + (kind[j] == PLAN_VAR_UPPER ? 1 : 0)), 0, 0, (int32_t)kind[j]};
        if (kind[j] == PLAN_VAR_FREE) {
            v.neg = (int32_t)(1 + ns + f);
            var[ns + f] = GVar{(int32_t)(2 * j + 1), 0, 0, (int32_t)PLAN_VAR_FREE};
            ++f;
        }
        if (kind[j] == PLAN_VAR_BOXED) {
            v.brow = (int32_t)(1 + m + t);
            bvar[m + t] = (int32_t)j;
            ++t;
        }
        var[j] = v;
    }
    return 0;
}

// a flip of the sign bit: NaN payloads survive it
LPK_PLAN_HD inline double plan_flip(double v)
{
    unsigned long long u;
    __builtin_memcpy(&u, &v, sizeof u);
    u ^= 0x8000000000000000ull;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// One LP of a general batch in the packed layouts, every offset from the
// buffer's start: its tableau (toff), its m' rows (boff; the shifted column has
// one more entry per LP, so it starts at boff + lp), its x' (coff), its general
// block (poff), its var table (xoff), its slack and bvar tables (soff), and the
// caller's variables (voff) and rows (yoff).
struct GeneralLp {
    long long toff, boff, coff, poff, xoff, soff, voff, yoff;
    int m, mp, np, ns, nf, maximise;
};
// what lp_general_set_form keeps per LP of a ragged batch
struct GInfo {
    long long poff, xoff, voff, yoff;
    int32_t m, ns, nf, maximise;
};
// doubles of one general block: P, then lb[ns], then ub[ns]
LPK_PLAN_HD inline long long plan_general_block(long long m, long long ns) { return (m + 1) * (ns + 1) + 2 * ns; }

// One lane of the shift kernel: entry `row` of LP's shifted column from its
// general block.  Row 0 is the z cell, rows 1..m the right-hand sides, each a
// sequential loop over the shifted variables j ascending with every product
// rounded before the subtraction; a row above m is the range ub - lb of the
// BOXED variable bvar.  var(j) is the LP's table entry of variable j.
template <class Var>
LPK_PLAN_HD inline double plan_general_shift(int row, int m, int ns, bool maximise, const double *blk, Var var,
                                             int bvar)
{
    const double *lb = blk + (long long)(m + 1) * (ns + 1), *ub = lb + ns;
    if (row > m) return ub[bvar] - lb[bvar];
    const double *p = blk + (long long)row * (ns + 1);
    double acc = row == 0 && maximise ? plan_flip(p[0]) : p[0];
    for (int j = 0; j < ns; ++j) {
        const int kind = var(j).kind;
        if (kind == PLAN_VAR_PLAIN || kind == PLAN_VAR_FREE) continue;
        const double s = kind == PLAN_VAR_UPPER ? ub[j] : lb[j];
        const double a = row == 0 && maximise ? plan_flip(p[1 + j]) : p[1 + j];
        const double prod = a * s;
        acc = acc - prod;
    }
    return acc;
}

// what cell (row, col) of a general LP's standard-form tableau holds.  v is the
// var entry of col where 1 <= col <= nv = ns + nf, slack_of_row the row's slack
// entry where col > nv and row > 0; *srccol the block column a staged cell reads.
constexpr int PLAN_CELL_STAGED_FLIP = 4, PLAN_CELL_SHIFTED = 5, PLAN_CELL_RANGE = 6;
LPK_PLAN_HD inline int plan_general_cell(int row, int col, int m, int nv, bool maximise, GVar v, int slack_of_row,
                                         int *srccol)
{
    *srccol = 0;
    if (col == 0) return row <= m ? PLAN_CELL_SHIFTED : PLAN_CELL_RANGE;
    if (col <= nv) {
        if (row > m) return v.brow == row ? PLAN_CELL_PLUS : PLAN_CELL_ZERO;
        *srccol = 1 + (v.src >> 1);
        const bool f = (v.src & 1) != 0;
        return (row == 0 ? maximise != f : f) ? PLAN_CELL_STAGED_FLIP : PLAN_CELL_STAGED;
    }
    if (row == 0) return PLAN_CELL_ZERO;
    return slack_of_row == col ? PLAN_CELL_PLUS : slack_of_row == -col ? PLAN_CELL_MINUS : PLAN_CELL_ZERO;
}

// One lane of the general assembly, on the host and on the device: destination
// element e of a window of `elems` whose first LP's tableau starts at tbase.
// locate(e) is the LP of element e, shape(i) LP i's GeneralLp, var(at) and
// slack(at) table entries; put(e, kind, src) stores one cell: src indexes the
// staged blocks for PLAN_CELL_STAGED / _STAGED_FLIP, the shifted columns for
// PLAN_CELL_SHIFTED / _RANGE, and is -1 otherwise.
template <class Locate, class Shape, class VarAt, class Slack, class Put>
LPK_PLAN_HD inline void plan_general_lane(long long e, long long elems, long long tbase, Locate locate, Shape shape,
                                          VarAt var, Slack slack, Put put)
{
    if (e >= elems) return;
    const long long lp = locate(e);
    const GeneralLp L = shape(lp);
    const ProblemAt at = plan_problem_at(lp, e - (L.toff - tbase), L.np + 1);
    const int nv = L.ns + L.nf;
    GVar v{0, 0, 0, 0};
    if (at.col >= 1 && at.col <= nv) v = var(L.xoff + at.col - 1);
    const int s = at.col > nv && at.row > 0 ? slack(L.soff + at.row - 1) : 0;
    int sc = 0;
    const int kind = plan_general_cell(at.row, at.col, L.m, nv, L.maximise != 0, v, s, &sc);
    long long src = -1;
    if (kind == PLAN_CELL_STAGED || kind == PLAN_CELL_STAGED_FLIP) src = L.poff + (long long)at.row * (L.ns + 1) + sc;
    else if (kind == PLAN_CELL_SHIFTED || kind == PLAN_CELL_RANGE) src = L.boff + lp + at.row;
    put(e, kind, src);
}

// Recovery of one caller variable from x' (lp_solution_gather's values): the
// bits of x'_j for PLAIN, lb + x'_j for LOWER and BOXED, ub - x'_j for UPPER,
// x'_j - x'_neg for FREE (xneg is read for FREE only).
LPK_PLAN_HD inline double plan_general_x(int kind, double xj, double xneg, double lb, double ub)
{
    return kind == PLAN_VAR_PLAIN   ? xj
           : kind == PLAN_VAR_UPPER ? ub - xj
           : kind == PLAN_VAR_FREE  ? xj - xneg
                                    : lb + xj;
}
// a row's dual: k_duals' value from its slack entry s != 0 and row 0's cell
// under it, flipped iff maximise
LPK_PLAN_HD inline double plan_general_y(int s, double c, bool maximise)
{
    const double y = s > 0 ? plan_flip(c) : c;
    return maximise ? plan_flip(y) : y;
}
// a variable's reduced cost: row 0's cell q under its column, less the cell
// under its bound row's slack for BOXED (cb), flipped iff (maximise XOR UPPER)
LPK_PLAN_HD inline double plan_general_r(int kind, double q, double cb, bool maximise)
{
    if (kind == PLAN_VAR_BOXED) q = q - cb;
    return maximise != (kind == PLAN_VAR_UPPER) ? plan_flip(q) : q;
}

// Lane g of a launch that gives LP i of the window [first, first + count) the
// lanes from start(i) - start(first) on (ragged, start ascending strictly), or
// `stride` lanes each (uniform) -> the LP; *rem the lane's place within it.
template <bool RAGGED, class Start>
LPK_PLAN_HD inline long long plan_general_lane_lp(long long first, long long count, long long g, long long stride,
                                                  Start start, long long *rem)
{
    long long lp;
    if constexpr (RAGGED) {
        const long long base = start(first);
        lp = plan_lane_lp(first, first + count, g, [=](long long i) { return start(i) - base; });
        *rem = g - (start(lp) - base);
    } else {
        lp = first + g / stride;
        *rem = g - (lp - first) * stride;
    }
    return lp;
}

// the launches: one lane per entry of the window's shifted columns, per
// destination element, per caller variable plus one per LP (the objective), per
// caller row plus per caller variable
inline FlatGrid plan_general_grid(int64_t lanes) { return plan_flat_grid(lanes, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS); }

// ---------------------------------------------------------------------------
// Warm re-optimisation (lp_reopt_*): new costs on the stored
// tableaux, and a new border (c, b, lb, ub) on the stored general blocks.
//
// New costs: a stored tableau is primal feasible for any c, and its row 0 is
// the cost row less c_B . [rows 1..m], one short loop per tableau column.  A
// lane of k_cost is one (LP, column) pair of the window, columns 0..n_i, LP
// after LP: LP i's n_i + 1 lanes start at (coff(i) - coff(first)) + (i - first),
// which is also where its n_i + 1 doubles begin in the packed costs.
// ---------------------------------------------------------------------------

// the launch of k_cost over the window's `pairs` = columns + LPs lanes
inline FlatGrid plan_cost_grid(int64_t pairs) { return plan_flat_grid(pairs, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS); }

// lane g's place: the LP, its tableau column and where the LP's costs begin
struct CostAt {
    long long lp, base;
    int col;
};
// uniform batch: every LP has n + 1 lanes
LPK_PLAN_HD inline CostAt plan_cost_at(long long first, long long g, int n)
{
    const long long k = g / (n + 1);
    return CostAt{first + k, k * (n + 1), (int)(g - k * (n + 1))};
}
// ragged batch: start(i) is the lane LP i begins at, ascending from start(first) = 0
template <class Start>
LPK_PLAN_HD inline CostAt plan_cost_at(long long first, long long hi, long long g, Start start)
{
    const long long lp = plan_lane_lp(first, hi, g, start);
    const long long base = start(lp);
    return CostAt{lp, base, (int)(g - base)};
}

// one product and one difference of the loop below, each rounded to nearest on
// its own: never an fma (the host build is compiled with -ffp-contract=off)
LPK_PLAN_HD inline double plan_cost_msub(double acc, double c, double t)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsub_rn(acc, __dmul_rn(c, t));
#else
    const double p = c * t;
    return acc - p;
#endif
}

// The new T[0][j] of an LP with m rows and n columns: basis(r) is row r's
// basic column (an entry outside [0, n) is skipped), cell(r) the stored
// T[1+r][j] and cost(k) the LP's k-th new value, cost(0) the stored _z cell.
// Rows ascending: the order is the contract.
template <class Basis, class Cell, class Cost>
LPK_PLAN_HD inline double plan_cost_cell(int j, int m, int n, Basis basis, Cell cell, Cost cost)
{
    double acc = cost(j);
    for (int r = 0; r < m; ++r) {
        const int k = basis(r);
        if (k < 0 || k >= n) continue;
        acc = plan_cost_msub(acc, cost(1 + k), cell(r));
    }
    return acc;
}

// New border: the 3 ns + m + 1 doubles of an LP's border are row 0 of its
// block P (-c0, then c), then b, then lb, then ub.  Entry e of that -> where it
// lives in the stored general block (P row-major, then lb[ns], then ub[ns]).
LPK_PLAN_HD inline long long plan_restage_border(long long m, long long ns) { return 3 * ns + m + 1; }
LPK_PLAN_HD inline long long plan_restage_at(long long e, long long m, long long ns)
{
    if (e <= ns) return e;                                      // row 0 of P
    if (e <= ns + m) return (e - ns) * (ns + 1);                // b_i = P[1+i][0], i = e - ns - 1
    return (m + 1) * (ns + 1) + (e - ns - m - 1);               // lb, then ub: contiguous in both
}
inline FlatGrid plan_restage_grid(int64_t lanes) { return plan_flat_grid(lanes, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS); }

// ---------------------------------------------------------------------------
// Warm cuts (lp_cut_extend): the stored (m+1) x (n+1) tableaux
// of a source batch, q more rows each, written into a destination batch whose
// LPs are (m+q+1) x (n+q+1).  The old tableau keeps its bits, the q new slack
// columns are +0.0 above an identity, and each new row is the stated row
// priced out against the basis rows -- plan_cost_cell's loop written into row
// 1 + m + k instead of row 0.
//
// Both batches may be uniform or ragged, so the kernels take every offset
// from one table of the window's LPs, count + 1 entries in window order, which
// the host derives from the two layouts and stages with the rows; the last
// entry holds the totals.  The lookups below are plan_lane_lp over a column
// of that table: starts ascend, and where an LP has no lane (q = 0) its start
// equals the next one's, so the last entry at or below a lane owns it.
// ---------------------------------------------------------------------------
#ifndef LPK_CUT_GROUP
#define LPK_CUT_GROUP 4
#endif
constexpr int PLAN_CUT_GROUP = LPK_CUT_GROUP;
static_assert(PLAN_CUT_GROUP >= 1 && PLAN_CUT_GROUP <= 16, "new rows per lane of k_cut_rows");

struct CutLp {
    long long stoff, dtoff;     // the LP's tableau: doubles from the source's and the destination's T
    long long sboff, dboff;     // its basis: entries from the two packed bases
    long long e0;               // its first destination element, from the window's first
    long long b0;               // its first destination basis entry, from the window's first
    long long lane0;            // its first lane of k_cut_rows
    long long roff;             // its stated rows in the staged rows: q rows of n + 1 doubles
    long long qoff;             // its senses in the staged senses: q entries
    int32_t m, n, q, pad;       // the source's shape, and the rows added
};

// lanes of k_cut_rows an LP takes: one per (group of up to PLAN_CUT_GROUP new rows, column 0..n)
LPK_PLAN_HD inline long long plan_cut_lanes(long long n, long long q)
{
    return (q + PLAN_CUT_GROUP - 1) / PLAN_CUT_GROUP * (n + 1);
}

// the running offsets of the entry that follows `at` in the table (the rest is the next LP's own)
inline CutLp plan_cut_next(const CutLp &at)
{
    CutLp nx{};
    nx.e0 = at.e0 + (long long)(at.m + at.q + 1) * (at.n + at.q + 1);
    nx.b0 = at.b0 + at.m + at.q;
    nx.lane0 = at.lane0 + plan_cut_lanes(at.n, at.q);
    nx.roff = at.roff + (long long)at.q * (at.n + 1);
    nx.qoff = at.qoff + at.q;
    return nx;
}

// the launches: k_cut_copy over the window's destination elements, k_cut_rows
// over its lanes, k_cut_basis over its destination basis entries
inline FlatGrid plan_cut_copy_grid(int64_t elems) { return plan_assemble_grid(elems); }
inline FlatGrid plan_cut_grid(int64_t lanes) { return plan_flat_grid(lanes, PLAN_FLAT_THREADS, PLAN_FLAT_THREADS); }

// what cell (row, col) of a destination tableau holds; src is the cell's
// offset in the source tableau for PLAN_CUT_COPY and 0 otherwise
constexpr int PLAN_CUT_COPY = 0, PLAN_CUT_ZERO = 1, PLAN_CUT_ONE = 2, PLAN_CUT_PRICED = 3;
struct CutCell {
    int kind;
    long long src;
};
LPK_PLAN_HD inline CutCell plan_cut_cell(int row, int col, int m, int n)
{
    if (row <= m) {
        if (col <= n) return CutCell{PLAN_CUT_COPY, (long long)row * (n + 1) + col};
        return CutCell{PLAN_CUT_ZERO, 0};
    }
    if (col <= n) return CutCell{PLAN_CUT_PRICED, 0};
    return CutCell{col - n == row - m ? PLAN_CUT_ONE : PLAN_CUT_ZERO, 0};
}

// One lane of k_cut_copy, on the host and on the device: the PLAN_ASSEMBLE_RUN
// destination elements from `e0` of a window of `elems`.  locate(e) is the
// table index of element e's LP, lp(k) entry k; put(dst, kind, src) stores one
// cell, dst and src doubles from the two batches' T (a PLAN_CUT_PRICED cell
// is passed on too: the kernel skips it; src is read for PLAN_CUT_COPY only).
template <class Locate, class Lp, class Put>
LPK_PLAN_HD inline void plan_cut_lane(long long e0, long long elems, Locate locate, Lp lp, Put put)
{
    if (e0 >= elems) return;
    const long long k0 = locate(e0);
    CutLp L = lp(k0);
    ProblemAt at = plan_problem_at(k0, e0 - L.e0, L.n + L.q + 1);
    for (int r = 0; r < PLAN_ASSEMBLE_RUN; ++r) {
        const long long e = e0 + r;
        if (e >= elems) return;
        const CutCell c = plan_cut_cell(at.row, at.col, L.m, L.n);
        put(L.dtoff + (e - L.e0), c.kind, L.stoff + c.src);
        if (plan_problem_next(at, L.m + L.q, L.n + L.q) && e + 1 < elems) L = lp(at.lp);
    }
}

// lane `local` of an LP's lanes of k_cut_rows -> its group's first new row and its column
struct CutAt {
    int k0, col;
};
LPK_PLAN_HD inline CutAt plan_cut_at(long long local, int n)
{
    const long long g = local / (n + 1);
    return CutAt{(int)g * PLAN_CUT_GROUP, (int)(local - g * (n + 1))};
}

// the accumulators of plan_cut_rows live in registers: its loops over them are unrolled on the device
#ifdef __HIP__
#define LPK_PLAN_UNROLL _Pragma("unroll")
#else
#define LPK_PLAN_UNROLL
#endif

// a value with its sign bit flipped: a >= cut is stored negated, NaN payloads and zeros included
LPK_PLAN_HD inline double plan_cut_flip(double v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double(__double_as_longlong(v) ^ (long long)(1ull << 63));
#else
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    b ^= 1ull << 63;
    __builtin_memcpy(&v, &b, sizeof b);
    return v;
#endif
}

// Column j of the new rows [k0, k1), k1 - k0 <= G, of an LP with m rows and n
// columns: basis(r) is row r's basic column (an entry outside [0, n) is
// skipped), cell(r) the stored T[1+r][j], row(k, c) cell c of stated row k
// (c = 0: beta).  The column is walked once, rows ascending, one accumulator
// per new row: each sees plan_cost_cell's order, whatever G is.  put(k, acc)
// takes the priced cell of row k, before any flip.
template <int G, class Basis, class Cell, class Row, class Put>
LPK_PLAN_HD inline void plan_cut_rows(int j, int m, int n, int k0, int k1, Basis basis, Cell cell, Row row, Put put)
{
    double acc[G];
    LPK_PLAN_UNROLL
    for (int g = 0; g < G; ++g) acc[g] = k0 + g < k1 ? row(k0 + g, j) : 0.0;
    for (int r = 0; r < m; ++r) {
        const int c = basis(r);
        if (c < 0 || c >= n) continue;
        const double t = cell(r);
    LPK_PLAN_UNROLL
        for (int g = 0; g < G; ++g)
            if (k0 + g < k1) acc[g] = plan_cost_msub(acc[g], row(k0 + g, 1 + c), t);
    }
    LPK_PLAN_UNROLL
    for (int g = 0; g < G; ++g)
        if (k0 + g < k1) put(k0 + g, acc[g]);
}

}  // namespace lpk
