// Host-only driver of the phased placement rule and plan (batch_plan.h:
// plan_place_phased, plan_phased_lds, plan_phased_chunk, plan_phased) for
// tests/test_batch_phase_cpu.py: one request per line on stdin, one answer per
// line on stdout.
//
//   place place= m= n=
//       -> where= plain= tplds= phlds=     (plain: plan_place's answer)
//   chunk chunk= work= m= n=
//       -> pivots=
//   plan place= cap1= cap4= elems= dwaves= dcap= shapes=m:n,m:n,...
//       -> too_large=I bins=D:WAVES:LDS:PER_CU:i.i.i;D:WAVES:LDS:PER_CU:i.i;...
//          (D = 1: the bin of the device-placed LPs)
//   ragged cap1= cap4= elems= shapes=...
//       -> the same line from plan_ragged (two-phase), for comparison
//
// cap1 / cap4 / dcap stand in for the runtime's occupancy answers at zero
// dynamic LDS, elems for the one-wave threshold, dwaves for the waves per
// device-placed LP.
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
        std::fprintf(stderr, "batch_phase_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

void shapes(std::vector<int64_t> &m, std::vector<int64_t> &n)
{
    std::istringstream sh(field("shapes"));
    std::string one;
    while (std::getline(sh, one, ',')) {
        const size_t c = one.find(':');
        if (c == std::string::npos) {
            std::fprintf(stderr, "batch_phase_check: shape %s\n", one.c_str());
            std::exit(2);
        }
        m.push_back(std::atoll(one.substr(0, c).c_str()));
        n.push_back(std::atoll(one.substr(c + 1).c_str()));
    }
}

void print_plan(const BatchPlan &P)
{
    std::printf("too_large=%lld bins=", (long long)P.too_large);
    for (size_t b = 0; b < P.bins.size(); ++b) {
        const PlanBin &B = P.bins[b];
        std::printf("%s%d:%d:%lld:%d:", b ? ";" : "", B.device ? 1 : 0, B.waves, (long long)B.lds, B.lps_per_cu);
        for (size_t k = 0; k < B.order.size(); ++k) std::printf("%s%d", k ? "." : "", (int)B.order[k]);
    }
    std::printf("\n");
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
                std::fprintf(stderr, "batch_phase_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "place") {
            const long long m = num("m"), n = num("n");
            const int place = (int)num("place");
            std::printf("where=%d plain=%d tplds=%lld phlds=%lld\n", plan_place_phased(place, m, n),
                        plan_place(place, m, n), (long long)plan_twophase_lds(m, n), (long long)plan_phased_lds(m, n));
        } else if (what == "chunk") {
            std::printf("pivots=%lld\n", (long long)plan_phased_chunk(num("chunk"), num("work"), num("m"), num("n")));
        } else if (what == "plan" || what == "ragged") {
            std::vector<int64_t> m, n;
            shapes(m, n);
            if (what == "plan")
                print_plan(plan_phased((int64_t)m.size(), m.data(), n.data(), (int)num("place"), (int)num("cap1"),
                                       (int)num("cap4"), num("elems"), (int)num("dwaves"), (int)num("dcap")));
            else
                print_plan(plan_ragged((int64_t)m.size(), m.data(), n.data(), true, (int)num("cap1"),
                                       (int)num("cap4"), num("elems")));
        } else {
            std::fprintf(stderr, "batch_phase_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
