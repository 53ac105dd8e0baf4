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

}  // namespace lpk
