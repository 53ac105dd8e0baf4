// Host-only driver of the warm re-solve's rules (batch_plan.h: plan_rhs_grid,
// plan_rhs_at, plan_rhs_cell) for tests/test_batch_rhs_cpu.py: one request per
// line on stdin, one answer per line on stdout.
//
//   grid pairs=
//       -> blocks= threads=     (blocks = -1: more than a grid holds)
//   cell row= slack=a,b,... cells=hex,hex,... rhs=hex,hex,...
//       -> acc=hex
//          plan_rhs_cell on one tableau row given as its n + 1 cells (cell 0 is
//          not read) and the LP's m + 1 new values, all as 64-bit patterns
//   sweep shapes=m:n,m:n,... senses=01/10/... first= count= uniform=0|1
//       -> pairs= bad_map= bad_cells= bad_rest=
//          every lane of the window's launch walked with plan_rhs_at and
//          plan_rhs_cell: bad_map counts (LP, row) pairs of the window not
//          visited exactly once, visited from outside it, or visited with
//          another rhs base than the packed layout gives; bad_cells the new
//          column-0 cells whose 64 bits differ from the loop written out;
//          bad_rest the cells outside column 0 of the window, or anywhere
//          outside the window, that a lane would have changed.  uniform=1: one
//          shape, the divisions of a uniform batch.
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
        std::fprintf(stderr, "batch_rhs_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
long long num(const char *name) { return std::atoll(field(name).c_str()); }

std::vector<std::string> split(const std::string &text, char sep)
{
    std::vector<std::string> out;
    std::istringstream in(text);
    std::string one;
    while (std::getline(in, one, sep)) out.push_back(one);
    return out;
}

double from_hex(const std::string &h)
{
    const uint64_t bits = std::strtoull(h.c_str(), nullptr, 16);
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

uint64_t bits_of(double v)
{
    uint64_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    return bits;
}

// distinct dyadic values of both signs with a -0.0 among them; never NaN, so a changed cell shows
double cell_value(int64_t lp, int64_t at)
{
    if (at % 29 == 7) return -0.0;
    return (double)(at % 97 + 1) * (at % 2 ? -0.0625 : 0.1875) + (double)(lp % 13) * 0.5;
}

int cell()
{
    std::vector<int> slack;
    for (const std::string &s : split(field("slack"), ',')) slack.push_back(std::atoi(s.c_str()));
    std::vector<double> cells, rhs;
    for (const std::string &s : split(field("cells"), ',')) cells.push_back(from_hex(s));
    for (const std::string &s : split(field("rhs"), ',')) rhs.push_back(from_hex(s));
    const int m = (int)slack.size();
    if ((int)rhs.size() != m + 1) return 2;
    for (int s : slack)
        if (s == 0 || std::abs(s) >= (int)cells.size()) return 2;
    const double acc = plan_rhs_cell(
        (int)num("row"), m, [&](int k) { return slack[(size_t)k]; }, [&](int c) { return cells[(size_t)c]; },
        [&](int k) { return rhs[(size_t)k]; });
    std::printf("acc=%016llx\n", (unsigned long long)bits_of(acc));
    return 0;
}

int sweep()
{
    std::vector<int64_t> m, n;
    for (const std::string &one : split(field("shapes"), ',')) {
        const size_t c = one.find(':');
        if (c == std::string::npos) return 2;
        m.push_back(std::atoll(one.substr(0, c).c_str()));
        n.push_back(std::atoll(one.substr(c + 1).c_str()));
    }
    std::vector<std::vector<int8_t>> sense;
    for (const std::string &one : split(field("senses"), '/')) {
        std::vector<int8_t> s;
        for (char c : one) s.push_back((int8_t)(c - '0'));
        sense.push_back(s);
    }
    const int64_t count = (int64_t)m.size();
    const bool uniform = num("uniform") != 0;
    if (sense.size() != (size_t)count) return 2;
    // the batch's tables, as lp_problem_set_senses derives them
    std::vector<int64_t> toff((size_t)count + 1), boff((size_t)count + 1);
    std::vector<int32_t> slack;
    for (int64_t i = 0; i < count; ++i) {
        const size_t u = (size_t)i;
        if ((int64_t)sense[u].size() != m[u]) return 2;
        if (uniform && (m[u] != m[0] || n[u] != n[0] || sense[u] != sense[0])) return 2;
        std::vector<int32_t> tab((size_t)m[u]);
        if (plan_problem_slack(sense[u].data(), m[u], n[u], tab.data()) < 0) return 2;
        for (int32_t s : tab)
            if (s == 0) return 2;               // an equality: the call refuses the LP
        if (!uniform || i == 0) slack.insert(slack.end(), tab.begin(), tab.end());
        toff[u + 1] = toff[u] + (m[u] + 1) * (n[u] + 1);
        boff[u + 1] = boff[u] + m[u];
    }
    const int64_t first = num("first"), cnt = num("count");
    if (first < 0 || cnt < 1 || first + cnt > count) return 2;
    // the whole batch's tableaux and the window's packed rhs
    std::vector<double> T((size_t)toff[(size_t)count]);
    for (int64_t i = 0; i < count; ++i)
        for (int64_t e = 0; e < toff[(size_t)i + 1] - toff[(size_t)i]; ++e)
            T[(size_t)(toff[(size_t)i] + e)] = cell_value(i, e);
    const int64_t pairs = boff[(size_t)(first + cnt)] - boff[(size_t)first] + cnt;
    std::vector<double> rhs((size_t)pairs);
    for (int64_t k = 0; k < pairs; ++k) rhs[(size_t)k] = cell_value(first + 5, 3 * k + 1);
    // the loop written out
    std::vector<double> want = T;
    for (int64_t i = first; i < first + cnt; ++i) {
        const size_t u = (size_t)i;
        const int64_t w = n[u] + 1, base = boff[u] - boff[(size_t)first] + (i - first);
        const int32_t *tab = slack.data() + (uniform ? 0 : boff[u]);
        for (int64_t row = 0; row <= m[u]; ++row) {
            double acc = row == 0 ? rhs[(size_t)base] : 0.0;
            for (int64_t k = 0; k < m[u]; ++k) {
                const int64_t col = tab[k] > 0 ? tab[k] : -tab[k];
                const double t = T[(size_t)(toff[u] + row * w + col)];
                const double p = (tab[k] > 0 ? t : -t) * rhs[(size_t)(base + 1 + k)];
                acc = acc + p;
            }
            want[(size_t)(toff[u] + row * w)] = acc;
        }
    }
    // every lane of the launch
    const FlatGrid g = plan_rhs_grid(pairs);
    std::vector<double> got = T;
    std::vector<int> hits((size_t)(boff[(size_t)count] + count), 0);
    long long bad_map = 0;
    for (int64_t lane = 0; lane < g.blocks * g.threads; ++lane) {
        if (lane >= pairs) continue;            // the kernel's bound
        const RhsAt at = uniform ? plan_rhs_at(first, lane, (int)m[0])
                                 : plan_rhs_at(first, first + cnt, lane, [&](long long i) {
                                       return (long long)(boff[(size_t)i] - boff[(size_t)first] + (i - first));
                                   });
        if (at.lp < first || at.lp >= first + cnt || at.row < 0 || at.row > m[(size_t)at.lp] ||
            at.base != boff[(size_t)at.lp] - boff[(size_t)first] + (at.lp - first)) {
            ++bad_map;
            continue;
        }
        const size_t u = (size_t)at.lp;
        ++hits[(size_t)(boff[u] + at.lp + at.row)];
        const double *row = T.data() + toff[u] + (int64_t)at.row * (n[u] + 1);
        const int32_t *tab = slack.data() + (uniform ? 0 : boff[u]);
        const double *r = rhs.data() + at.base;
        got[(size_t)(toff[u] + (int64_t)at.row * (n[u] + 1))] = plan_rhs_cell(
            at.row, (int)m[u], [&](int k) { return (int)tab[k]; }, [&](int c) { return row[c]; },
            [&](int k) { return r[k]; });
    }
    long long bad_cells = 0, bad_rest = 0;
    for (int64_t i = 0; i < count; ++i) {
        const size_t u = (size_t)i;
        const bool in = i >= first && i < first + cnt;
        for (int64_t row = 0; row <= m[u]; ++row) {
            if (hits[(size_t)(boff[u] + i + row)] != (in ? 1 : 0)) ++bad_map;
            for (int64_t col = 0; col <= n[u]; ++col) {
                const size_t e = (size_t)(toff[u] + row * (n[u] + 1) + col);
                const bool same = bits_of(got[e]) == bits_of(want[e]);
                if (in && col == 0) bad_cells += same ? 0 : 1;
                else bad_rest += same && bits_of(got[e]) == bits_of(T[e]) ? 0 : 1;
            }
        }
    }
    std::printf("pairs=%lld bad_map=%lld bad_cells=%lld bad_rest=%lld\n", (long long)pairs, bad_map, bad_cells,
                bad_rest);
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
                std::fprintf(stderr, "batch_rhs_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        int st = 0;
        if (what == "grid") {
            const FlatGrid g = plan_rhs_grid(num("pairs"));
            std::printf("blocks=%lld threads=%d\n", (long long)g.blocks, g.threads);
        } else if (what == "cell") {
            st = cell();
        } else if (what == "sweep") {
            st = sweep();
        } else {
            std::fprintf(stderr, "batch_rhs_check: request %s\n", what.c_str());
            return 2;
        }
        if (st) {
            std::fprintf(stderr, "batch_rhs_check: bad %s request\n", what.c_str());
            return st;
        }
    }
    return 0;
}
