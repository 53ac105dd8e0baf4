// Host-only driver of the team rules (batch_plan.h: plan_team_size,
// plan_team_ranges, plan_team_table) for tests/test_batch_team_cpu.py: one
// request per line on stdin, one answer per line on stdout.
//
//   size request= ndev= m= n= slots= max= min= lpe=   (lpe = 0: teams whatever ndev is)
//       -> team=            (-1: refused)
//   ranges E= toff= G=
//       -> ends=e0.e1. ... .eG
//   sweep Emax= Gmax=
//       -> checked= bad=    every E in 2..Emax x toff parity x G in 1..min(Gmax, E/2):
//                           coverage, order, no empty range, even interior ends,
//                           pair counts within one of each other
//   table shapes=m:n,m:n,... teams=g,g,...
//       -> wgs=LP:RANK:G:E0:E1;...   (the LPs packed back to back, as a ragged batch keeps them)
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
        std::fprintf(stderr, "batch_team_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

// what plan_team_ranges promises, for one (E, toff, G)
bool ranges_ok(int64_t E, int64_t toff, int G)
{
    const std::vector<int64_t> e = plan_team_ranges(E, toff, G);
    if ((int)e.size() != G + 1 || e[0] != 0 || e[(size_t)G] != E) return false;
    int64_t least = INT64_MAX, most = 0;
    for (int r = 0; r < G; ++r) {
        const int64_t a = e[(size_t)r], b = e[(size_t)r + 1];
        if (b <= a) return false;                               // in order, none empty
        if (r > 0 && ((toff + a) & 1)) return false;            // interior ends at pair boundaries
        const int64_t pairs = (toff + b - 1) / 2 - (toff + a) / 2 + 1;
        least = std::min(least, pairs);
        most = std::max(most, pairs);
    }
    return most - least <= 1;
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
                std::fprintf(stderr, "batch_team_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "size") {
            std::printf("team=%d\n", plan_team_size((int)num("request"), num("ndev"), num("m"), num("n"), num("slots"),
                                                    (int)num("max"), num("min"), num("lpe")));
        } else if (what == "ranges") {
            const std::vector<int64_t> e = plan_team_ranges(num("E"), num("toff"), (int)num("G"));
            std::printf("ends=");
            for (size_t k = 0; k < e.size(); ++k) std::printf("%s%lld", k ? "." : "", (long long)e[k]);
            std::printf("\n");
        } else if (what == "sweep") {
            long long checked = 0, bad = 0;
            for (int64_t E = 2; E <= num("Emax"); ++E)
                for (int64_t toff = 0; toff < 2; ++toff)
                    for (int G = 1; G <= std::min<int64_t>(num("Gmax"), E / 2); ++G) {
                        ++checked;
                        // an odd base far from zero: the same cuts as its parity
                        if (!ranges_ok(E, toff, G) || plan_team_ranges(E, toff + 1000, G) != plan_team_ranges(E, toff, G))
                            ++bad;
                    }
            std::printf("checked=%lld bad=%lld\n", checked, bad);
        } else if (what == "table") {
            std::vector<int64_t> m, n, toff;
            std::vector<int32_t> team;
            std::istringstream sh(field("shapes")), tm(field("teams"));
            std::string one;
            int64_t at = 0;
            while (std::getline(sh, one, ',')) {
                const size_t c = one.find(':');
                if (c == std::string::npos) return 2;
                m.push_back(std::atoll(one.substr(0, c).c_str()));
                n.push_back(std::atoll(one.substr(c + 1).c_str()));
                toff.push_back(at);
                at += (m.back() + 1) * (n.back() + 1);
            }
            while (std::getline(tm, one, ',')) team.push_back((int32_t)std::atoi(one.c_str()));
            if (team.size() != m.size()) return 2;
            const std::vector<TeamWG> wg = plan_team_table((int64_t)m.size(), m.data(), n.data(), toff.data(), team.data());
            std::printf("wgs=");
            for (size_t k = 0; k < wg.size(); ++k)
                std::printf("%s%d:%d:%d:%d:%d", k ? ";" : "", wg[k].lp, wg[k].rank, wg[k].G, wg[k].e0, wg[k].e1);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "batch_team_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
