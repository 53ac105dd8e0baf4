// Host-only driver of the problem-form batches' rules (batch_plan.h:
// plan_problem_slack, plan_assemble_grid, plan_assemble_lane and what it
// calls) for tests/test_batch_problem_cpu.py: one request per line on stdin,
// one answer per line on stdout.
//
//   table senses=0120 n=
//       -> ns= table=a,b,...     ns < 0: refused (-1 bad sense with row=, -2 no
//                                structural variable, -3 bad shape), table=- and
//                                the output buffer untouched (untouched=1)
//   grid elems=
//       -> blocks= threads= run=     (blocks = -1: more than a grid holds)
//   sweep shapes=m:n,m:n,... senses=01/2/... first= count= uniform=0|1
//       -> elems= lanes= bad_map= bad_cells=
//          every lane of the window's launch walked with plan_assemble_lane:
//          bad_map counts destination elements not written exactly once or
//          written from another (kind, source) than a plain walk over the LPs,
//          rows and columns gives; bad_cells the 64-bit cells in which the
//          tableaux assembled through the lanes differ from the formula written
//          out.  uniform=1: one shape, the divisions of a uniform batch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        std::fprintf(stderr, "batch_problem_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

std::vector<int8_t> senses_of(const std::string &digits)
{
    std::vector<int8_t> s;
    for (char c : digits) s.push_back((int8_t)(c - '0'));
    return s;
}

double staged_value(int64_t lp, int64_t at)
{
    // distinct, with both signs, a -0.0 and a NaN with a payload among them
    if (at % 29 == 7) return -0.0;
    if (at % 31 == 11) {
        const uint64_t bits = 0x7ff8000000000000ull | (uint64_t)(1 + lp % 1000);
        double v;
        std::memcpy(&v, &bits, sizeof v);
        return v;
    }
    return (double)(at + 1) * (at % 2 ? -0.25 : 0.5) + (double)lp * 4096.0;
}

int sweep()
{
    std::vector<int64_t> m, n;
    std::istringstream sh(field("shapes"));
    std::string one;
    while (std::getline(sh, one, ',')) {
        const size_t c = one.find(':');
        if (c == std::string::npos) return 2;
        m.push_back(std::atoll(one.substr(0, c).c_str()));
        n.push_back(std::atoll(one.substr(c + 1).c_str()));
    }
    std::vector<std::vector<int8_t>> sense;
    std::istringstream ss(field("senses"));
    while (std::getline(ss, one, '/')) sense.push_back(senses_of(one));
    const int64_t count = (int64_t)m.size();
    const bool uniform = num("uniform") != 0;
    if (sense.size() != (size_t)count) return 2;
    // the batch's tables, as lp_problem_set_senses derives them
    std::vector<int64_t> toff((size_t)count + 1), boff((size_t)count + 1), poff((size_t)count + 1), ns((size_t)count);
    std::vector<int32_t> slack;
    for (int64_t i = 0; i < count; ++i) {
        if ((int64_t)sense[(size_t)i].size() != m[(size_t)i]) return 2;
        if (uniform && (m[(size_t)i] != m[0] || n[(size_t)i] != n[0] || sense[(size_t)i] != sense[0])) return 2;
        std::vector<int32_t> tab((size_t)m[(size_t)i]);
        ns[(size_t)i] = plan_problem_slack(sense[(size_t)i].data(), m[(size_t)i], n[(size_t)i], tab.data());
        if (ns[(size_t)i] < 0) return 2;
        if (!uniform || i == 0) slack.insert(slack.end(), tab.begin(), tab.end());
        toff[(size_t)i + 1] = toff[(size_t)i] + (m[(size_t)i] + 1) * (n[(size_t)i] + 1);
        boff[(size_t)i + 1] = boff[(size_t)i] + m[(size_t)i];
        poff[(size_t)i + 1] = poff[(size_t)i] + (m[(size_t)i] + 1) * (ns[(size_t)i] + 1);
    }
    const int64_t first = num("first"), cnt = num("count");
    if (first < 0 || cnt < 1 || first + cnt > count) return 2;
    const int64_t tbase = toff[(size_t)first], pbase = poff[(size_t)first];
    const int64_t elems = toff[(size_t)(first + cnt)] - tbase, pelems = poff[(size_t)(first + cnt)] - pbase;
    // the staged blocks of the window and the formula written out
    std::vector<double> src((size_t)pelems), want((size_t)elems, 0.0);
    std::vector<int> want_kind((size_t)elems, PLAN_CELL_ZERO);
    std::vector<int64_t> want_src((size_t)elems, -1);
    for (int64_t i = first; i < first + cnt; ++i) {
        const int64_t w = n[(size_t)i] + 1, pw = ns[(size_t)i] + 1;
        const int64_t t0 = toff[(size_t)i] - tbase, p0 = poff[(size_t)i] - pbase;
        for (int64_t k = 0; k < (m[(size_t)i] + 1) * pw; ++k) src[(size_t)(p0 + k)] = staged_value(i, k);
        int64_t t = 0;
        for (int64_t row = 0; row <= m[(size_t)i]; ++row) {
            for (int64_t col = 0; col < w; ++col) want_src[(size_t)(t0 + row * w + col)] = p0 + row * pw + col;
            for (int64_t col = 0; col < pw; ++col) {
                want[(size_t)(t0 + row * w + col)] = src[(size_t)(p0 + row * pw + col)];
                want_kind[(size_t)(t0 + row * w + col)] = PLAN_CELL_STAGED;
            }
            if (row == 0 || sense[(size_t)i][(size_t)(row - 1)] == PLAN_SENSE_EQ) continue;
            const bool le = sense[(size_t)i][(size_t)(row - 1)] == PLAN_SENSE_LE;
            want[(size_t)(t0 + row * w + pw + t)] = le ? 1.0 : -1.0;
            want_kind[(size_t)(t0 + row * w + pw + t)] = le ? PLAN_CELL_PLUS : PLAN_CELL_MINUS;
            ++t;
        }
    }
    // every lane of the launch
    const FlatGrid g = plan_assemble_grid(elems);
    std::vector<double> got((size_t)elems, -7.0);
    std::vector<int> hits((size_t)elems, 0);
    long long bad_map = 0;
    const int64_t E0 = (m[0] + 1) * (n[0] + 1), P0 = (m[0] + 1) * (ns[0] + 1);
    auto put = [&](long long e, int kind, long long at) {
        if (e < 0 || e >= elems) {
            ++bad_map;
            return;
        }
        ++hits[(size_t)e];
        if (kind != want_kind[(size_t)e] || at != want_src[(size_t)e]) ++bad_map;
        got[(size_t)e] = kind == PLAN_CELL_STAGED ? src[(size_t)at]
                         : kind == PLAN_CELL_PLUS ? 1.0
                         : kind == PLAN_CELL_MINUS ? -1.0
                                                   : 0.0;
    };
    auto slack_at = [&](long long at) { return (int)slack[(size_t)at]; };
    for (int64_t lane = 0; lane < g.blocks * g.threads; ++lane) {
        if (uniform)
            plan_assemble_lane(
                lane * PLAN_ASSEMBLE_RUN, elems, [&](long long e) { return first + e / E0; },
                [&](long long i) {
                    return ProblemLp{(i - first) * E0, (i - first) * P0, 0, (int)m[0], (int)n[0], (int)ns[0]};
                },
                slack_at, put);
        else
            plan_assemble_lane(
                lane * PLAN_ASSEMBLE_RUN, elems,
                [&](long long e) {
                    return plan_lane_lp(first, first + cnt, e, [&](long long i) { return (long long)(toff[(size_t)i] - tbase); });
                },
                [&](long long i) {
                    return ProblemLp{toff[(size_t)i] - tbase, poff[(size_t)i] - pbase, boff[(size_t)i],
                                     (int)m[(size_t)i], (int)n[(size_t)i], (int)ns[(size_t)i]};
                },
                slack_at, put);
    }
    long long bad_cells = 0;
    for (int64_t e = 0; e < elems; ++e) {
        if (hits[(size_t)e] != 1) ++bad_map;
        if (std::memcmp(&got[(size_t)e], &want[(size_t)e], sizeof(double)) != 0) ++bad_cells;
    }
    std::printf("elems=%lld lanes=%lld bad_map=%lld bad_cells=%lld\n", (long long)elems, (long long)g.lanes, bad_map,
                bad_cells);
    return 0;
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
                std::fprintf(stderr, "batch_problem_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "table") {
            const std::vector<int8_t> s = senses_of(field("senses"));
            std::vector<int32_t> tab(s.size() + 1, 12345);
            int64_t row = -1;
            const int64_t ns = plan_problem_slack(s.empty() ? nullptr : s.data(), (int64_t)s.size(), num("n"),
                                                  tab.data(), &row);
            if (ns < 0) {
                bool untouched = true;
                for (int32_t v : tab) untouched = untouched && v == 12345;
                std::printf("ns=%lld row=%lld table=- untouched=%d\n", (long long)ns, (long long)row, untouched ? 1 : 0);
            } else {
                std::string t;
                for (size_t r = 0; r < s.size(); ++r) t += (r ? "," : "") + std::to_string(tab[r]);
                std::printf("ns=%lld row=-1 table=%s untouched=%d\n", (long long)ns, t.c_str(),
                            tab.back() == 12345 ? 1 : 0);
            }
        } else if (what == "grid") {
            const FlatGrid g = plan_assemble_grid(num("elems"));
            std::printf("blocks=%lld threads=%d run=%d\n", (long long)g.blocks, g.threads, PLAN_ASSEMBLE_RUN);
        } else if (what == "sweep") {
            const int st = sweep();
            if (st) {
                std::fprintf(stderr, "batch_problem_check: bad sweep request\n");
                return st;
            }
        } else {
            std::fprintf(stderr, "batch_problem_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
