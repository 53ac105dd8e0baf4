// Host-only driver of the solution batches' launch rules (batch_plan.h:
// plan_scan_slices, plan_scan_grid, plan_flat_grid, plan_lane_lp) for
// tests/test_batch_solution_plan_cpu.py: one request per line on stdin, one
// answer per line on stdout.
//
//   slices m=
//       -> slices=
//   scan cols= m=
//       -> blocks= threads= slices=     (blocks = -1: more than a grid holds)
//   flat lanes= per= threads=
//       -> blocks= threads=
//   sweep cols= m=
//       -> checked= bad=    every (c, mm) in 1..cols x 1..m: the grid covers the c lanes
//                           with no idle workgroup, threads = 64 x slices <= 1024
//   locate shapes=m:n,m:n,... first= count=
//       -> lanes= entries= bad=    every column lane and every basis entry of the window
//                                  found by plan_lane_lp against a walk over the LPs
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "batch_plan.h"

using namespace lpk;

namespace {

std::map<std::string, std::string> g_fields;

const std::string &field(const char *name)
{
    auto it = g_fields.find(name);
    if (it == g_fields.end()) {
        std::fprintf(stderr, "batch_solution_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

bool scan_ok(int64_t cols, int64_t m)
{
    const FlatGrid g = plan_scan_grid(cols, m);
    if (g.slices != plan_scan_slices(m) || g.slices < 1 || g.slices > PLAN_SCAN_MAX_SLICES) return false;
    if (g.threads != PLAN_SCAN_COLS * g.slices || g.threads > 1024) return false;
    return g.lanes == cols && g.blocks * PLAN_SCAN_COLS >= cols && (g.blocks - 1) * PLAN_SCAN_COLS < cols;
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, kv;
        if (!(in >> what)) continue;
        g_fields.clear();
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "batch_solution_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "slices") {
            std::printf("slices=%d\n", plan_scan_slices(num("m")));
        } else if (what == "scan") {
            const FlatGrid g = plan_scan_grid(num("cols"), num("m"));
            std::printf("blocks=%lld threads=%d slices=%d\n", (long long)g.blocks, g.threads, g.slices);
        } else if (what == "flat") {
            const FlatGrid g = plan_flat_grid(num("lanes"), (int)num("per"), (int)num("threads"));
            std::printf("blocks=%lld threads=%d\n", (long long)g.blocks, g.threads);
        } else if (what == "sweep") {
            long long checked = 0, bad = 0;
            for (int64_t c = 1; c <= num("cols"); ++c)
                for (int64_t m = 1; m <= num("m"); ++m) {
                    ++checked;
                    if (!scan_ok(c, m)) ++bad;
                }
            std::printf("checked=%lld bad=%lld\n", checked, bad);
        } else if (what == "locate") {
            std::vector<int64_t> m, n, coff, boff;
            std::istringstream sh(field("shapes"));
            std::string one;
            int64_t ca = 0, ba = 0;
            while (std::getline(sh, one, ',')) {
                const size_t c = one.find(':');
                if (c == std::string::npos) return 2;
                m.push_back(std::atoll(one.substr(0, c).c_str()));
                n.push_back(std::atoll(one.substr(c + 1).c_str()));
                coff.push_back(ca);
                boff.push_back(ba);
                ca += n.back();
                ba += m.back();
            }
            const int64_t first = num("first"), count = num("count");
            if (first < 0 || count < 1 || first + count > (int64_t)m.size()) return 2;
            long long lanes = 0, entries = 0, bad = 0;
            const int64_t cbase = coff[(size_t)first] + first, bbase = boff[(size_t)first];
            for (int64_t i = first; i < first + count; ++i) {
                for (int64_t jj = 0; jj <= n[(size_t)i]; ++jj, ++lanes) {
                    const long long got = plan_lane_lp(first, first + count, lanes, [&](long long k) {
                        return (long long)(coff[(size_t)k] + k - cbase);
                    });
                    if (got != i || lanes - (coff[(size_t)got] + got - cbase) != jj) ++bad;
                }
                for (int64_t r = 0; r < m[(size_t)i]; ++r, ++entries) {
                    const long long got = plan_lane_lp(first, first + count, entries, [&](long long k) {
                        return (long long)(boff[(size_t)k] - bbase);
                    });
                    if (got != i || entries - (boff[(size_t)got] - bbase) != r) ++bad;
                }
            }
            std::printf("lanes=%lld entries=%lld bad=%lld\n", lanes, entries, bad);
        } else {
            std::fprintf(stderr, "batch_solution_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
