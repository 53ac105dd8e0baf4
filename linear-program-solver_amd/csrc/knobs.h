// Every LPGPU_* environment knob of the engine, in one table (INTEGRATION.md
// lists them in this order).  Host only, no HIP include: parse_*_knobs take
// the lookup as a callback, so csrc/geometry_check.cpp parses NAME=VALUE pairs
// without touching the real environment.  (The Python loader's library path
// and bench.py's own variables are not the engine's and are not read here.)
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>

// Compile-time knobs of the teamed batch (csrc/batch.hip k_batch_team;
// DESIGN.md 4l), picked by scripts/team_sweep.py; an A/B build moves one with
// -DLPK_TEAM_...=.  They are not environment variables.
#ifndef LPK_TEAM_WAVES
#define LPK_TEAM_WAVES 8            // waves per workgroup of a team: 4, 8 or 16
#endif
#ifndef LPK_TEAM_MAX
#define LPK_TEAM_MAX 32             // the largest team
#endif
#ifndef LPK_TEAM_MIN_ELEMS
#define LPK_TEAM_MIN_ELEMS 1024     // auto: no range of a team below this many elements
#endif
#ifndef LPK_TEAM_LP_ELEMS
#define LPK_TEAM_LP_ELEMS 1500      // auto: no teams in a batch of more than E / this device-placed LPs
#endif
#ifndef LPK_TEAM_WINDOW
#define LPK_TEAM_WINDOW 64          // launches per read-back of the records (lp_teamed_set_window)
#endif

// New rows one lane of k_cut_rows prices out per walk of a source column
// (csrc/batch.hip); results do not depend on it.  batch_plan.h,
// which the host checks include alone, repeats the default.
#ifndef LPK_CUT_GROUP
#define LPK_CUT_GROUP 4
#endif

namespace lpk {

using KnobLookup = const char *(*)(const char *);

constexpr double SWEEP_SPLIT = 0.62;   // each CU's older sweep workgroup's share of the rows (plan_sweep_grid)

// Read once per process (process_knobs): tests set these through a child
// process's environment.
struct ProcessKnobs {
    int sweep_oop = 2;                       // LPGPU_SWEEP_OOP: 1 always, 0 never, unset (2): by size
    unsigned long long oop_room_mb = 1024;   // LPGPU_OOP_ROOM_MB (tests): headroom beyond the second buffer
    bool oop_fail_alloc = false;             // LPGPU_OOP_FAIL_ALLOC=1 (tests): the second buffer's allocation fails
    int sweep_cus = 0;                       // LPGPU_SWEEP_CUS (tests): > 0: the most CUs the sweep grid is sized for
    int sweep_tail = 1;                      // LPGPU_SWEEP_TAIL (tests): 0 no tail piece, 2 k_sweep_dp2's at any length
    double sweep_split = SWEEP_SPLIT;        // LPGPU_SWEEP_SPLIT (tests, A/B): 0 = equal runs
    int coop = 0;                            // LPGPU_COOP (tests): cooperative persistent launches
    int hier = 1;                            // LPGPU_HIER (A/B): 0 = flat exchange for spread blocks
    int gmaj = 1;                            // LPGPU_GMAJ (A/B): 0 = block-major summaries always
    bool ld_raw = false;                     // LPGPU_LD_RAW=1 (A/B): the plain rounded pitch
};

// Read at each handle's creation (lp_handle::knobs): tests change these
// between handles of one process.
struct HandleKnobs {
    bool persistent = true;            // LPGPU_SELECT=kernels: the per-pivot kernels only
    unsigned spin_max = 1u << 22;      // LPGPU_SPIN_MAX: polls of one k_group exchange before it gives up
    unsigned xwait_ms = 30000;         // LPGPU_XWAIT_MS: bound of a cross-rank wait (XR)
    int fault_launch = 0, fault_t = 0; // LPGPU_FAULT=<launch>:<pivot> (tests)
    int fault_xcc = 0;                 // LPGPU_FAULT_XCC=<launch> (tests): a block of k_sel reports another XCD
    bool strict = false;               // LPGPU_STRICT=1 (tests): a timed-out group is an error
    bool xs_ok = true;                 // LPGPU_SEL_XS=0 / lpdiag_set_xcd_shards: k_group instead of k_sel's XCD shards
    bool peer_enable = true;           // LPGPU_PEER=0 keeps the RCCL per-pivot path
    bool stamps = false;               // LPGPU_STAMPS=1 (diagnostic build): allocate the phase clocks
    int xr_xcd = -1;                   // LPGPU_XR_XCD (at lp_peer_open): -1 unset, 0 / 1 its first character, 2 other
};

inline ProcessKnobs parse_process_knobs(KnobLookup get)
{
    ProcessKnobs k;
    if (const char *v = get("LPGPU_SWEEP_OOP")) k.sweep_oop = std::atoi(v);
    if (const char *v = get("LPGPU_OOP_ROOM_MB")) k.oop_room_mb = std::strtoull(v, nullptr, 10);
    if (const char *v = get("LPGPU_OOP_FAIL_ALLOC")) k.oop_fail_alloc = v[0] == '1';
    if (const char *v = get("LPGPU_SWEEP_CUS")) k.sweep_cus = std::atoi(v);
    if (const char *v = get("LPGPU_SWEEP_TAIL")) k.sweep_tail = std::atoi(v);
    if (const char *v = get("LPGPU_SWEEP_SPLIT")) k.sweep_split = std::atof(v);
    if (const char *v = get("LPGPU_COOP")) k.coop = std::atoi(v);
    if (const char *v = get("LPGPU_HIER")) k.hier = std::atoi(v);
    if (const char *v = get("LPGPU_GMAJ")) k.gmaj = std::atoi(v);
    if (const char *v = get("LPGPU_LD_RAW")) k.ld_raw = v[0] == '1';
    return k;
}

inline HandleKnobs parse_handle_knobs(KnobLookup get)
{
    HandleKnobs k;
    if (const char *v = get("LPGPU_SELECT")) k.persistent = std::strcmp(v, "kernels") != 0;
    if (const char *v = get("LPGPU_SPIN_MAX")) k.spin_max = (unsigned)std::strtoul(v, nullptr, 10);
    if (const char *v = get("LPGPU_XWAIT_MS")) k.xwait_ms = (unsigned)std::strtoul(v, nullptr, 10);
    if (const char *v = get("LPGPU_FAULT")) std::sscanf(v, "%d:%d", &k.fault_launch, &k.fault_t);
    if (const char *v = get("LPGPU_FAULT_XCC")) k.fault_xcc = std::atoi(v);
    if (const char *v = get("LPGPU_STRICT")) k.strict = v[0] == '1';
    if (const char *v = get("LPGPU_SEL_XS")) k.xs_ok = v[0] != '0';
    if (const char *v = get("LPGPU_PEER")) k.peer_enable = v[0] != '0';
    if (const char *v = get("LPGPU_STAMPS")) k.stamps = v[0] == '1';
    if (const char *v = get("LPGPU_XR_XCD")) k.xr_xcd = v[0] == '0' ? 0 : v[0] == '1' ? 1 : 2;
    return k;
}

inline const char *knob_getenv(const char *name) { return std::getenv(name); }

inline const ProcessKnobs &process_knobs()
{
    static const ProcessKnobs k = parse_process_knobs(knob_getenv);
    return k;
}
inline HandleKnobs handle_knobs() { return parse_handle_knobs(knob_getenv); }

}  // namespace lpk
