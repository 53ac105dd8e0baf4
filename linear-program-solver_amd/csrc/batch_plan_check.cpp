// Host-only driver of the ragged-batch launch planner (batch_plan.h) for
// tests/test_ragged_plan_cpu.py: one request per line on stdin, one answer per
// line on stdout.
//
//   need m= n= elems=
//       -> plain= twophase= wplain= wtwophase=
//   plan kind=plain|twophase cap1= cap4= elems= shapes=m:n,m:n,...
//       -> too_large=I bins=WAVES:LDS:PER_CU:i.i.i;WAVES:LDS:PER_CU:i.i;...
//
// cap1 / cap4 stand in for the runtime's occupancy answer at zero dynamic LDS
// (workgroups per CU of the one-wave and the four-wave instantiation), elems
// for the one-wave threshold.
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
        std::fprintf(stderr, "batch_plan_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

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
                std::fprintf(stderr, "batch_plan_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "need") {
            const long long m = num("m"), n = num("n"), e = num("elems");
            std::printf("plain=%lld twophase=%lld wplain=%d wtwophase=%d\n", (long long)plan_plain_lds(m, n),
                        (long long)plan_twophase_lds(m, n), plan_plain_waves(m, n, e), plan_twophase_waves(m, n, e));
        } else if (what == "plan") {
            const std::string &kind = field("kind");
            if (kind != "plain" && kind != "twophase") {
                std::fprintf(stderr, "batch_plan_check: kind=%s\n", kind.c_str());
                return 2;
            }
            std::vector<int64_t> m, n;
            std::istringstream sh(field("shapes"));
            std::string one;
            while (std::getline(sh, one, ',')) {
                const size_t c = one.find(':');
                if (c == std::string::npos) {
                    std::fprintf(stderr, "batch_plan_check: shape %s\n", one.c_str());
                    return 2;
                }
                m.push_back(std::atoll(one.substr(0, c).c_str()));
                n.push_back(std::atoll(one.substr(c + 1).c_str()));
            }
            const BatchPlan P = plan_ragged((int64_t)m.size(), m.data(), n.data(), kind == "twophase",
                                            (int)num("cap1"), (int)num("cap4"), num("elems"));
            std::printf("too_large=%lld bins=", (long long)P.too_large);
            for (size_t b = 0; b < P.bins.size(); ++b) {
                const PlanBin &B = P.bins[b];
                std::printf("%s%d:%lld:%d:", b ? ";" : "", B.waves, (long long)B.lds, B.lps_per_cu);
                for (size_t k = 0; k < B.order.size(); ++k) std::printf("%s%d", k ? "." : "", (int)B.order[k]);
            }
            std::printf("\n");
        } else {
            std::fprintf(stderr, "batch_plan_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
