// Host-only driver of the warm re-optimisation's rules (batch_plan.h:
// plan_cost_grid, plan_cost_at, plan_cost_cell, plan_restage_at) for
// tests/test_batch_reopt_cpu.py: one request per line on stdin, one answer per
// line on stdout.
//
//   grid pairs=
//       -> blocks= threads=     (blocks = -1: more than a grid holds)
//   cell col= n= basis=a,b,... cells=hex,hex,... costs=hex,hex,...
//       -> acc=hex
//          plan_cost_cell on one tableau column given as its m cells of rows
//          1..m and the LP's n + 1 new values, all as 64-bit patterns
//   sweep shapes=m:n,m:n,... first= count= uniform=0|1
//       -> pairs= bad_map= bad_cells= bad_rest=
//          every lane of the window's launch walked with plan_cost_at and
//          plan_cost_cell: bad_map counts (LP, column) pairs of the window not
//          visited exactly once, visited from outside it, or visited with
//          another cost base than the packed layout gives; bad_cells the new
//          row-0 cells whose 64 bits differ from the loop written out;
//          bad_rest the cells outside row 0 of the window, or anywhere outside
//          the window, that a lane would have changed.  Every third basis
//          entry is -1 or n: skipped.  uniform=1: one shape, the divisions of
//          a uniform batch.
//   restage shapes=m:ns,m:ns,... first= count= uniform=0|1
//       -> lanes= bad_map= bad_cells= bad_rest=
//          every lane of k_general_restage's launch walked with
//          plan_general_lane_lp and plan_restage_at: bad_map counts border
//          cells of the window's blocks (row 0 of P, column 0 of rows 1..m,
//          lb, ub) not written exactly once; bad_cells those holding another
//          value than the border's; bad_rest the other cells of any block that
//          a lane would have changed.
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
        std::fprintf(stderr, "batch_reopt_check: field %s missing\n", name);
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

bool shapes(std::vector<int64_t> &a, std::vector<int64_t> &b, bool uniform)
{
    for (const std::string &one : split(field("shapes"), ',')) {
        const size_t c = one.find(':');
        if (c == std::string::npos) return false;
        a.push_back(std::atoll(one.substr(0, c).c_str()));
        b.push_back(std::atoll(one.substr(c + 1).c_str()));
        if (a.back() < 1 || b.back() < 1) return false;
        if (uniform && (a.back() != a[0] || b.back() != b[0])) return false;
    }
    return !a.empty();
}

int cell()
{
    std::vector<int> basis;
    for (const std::string &s : split(field("basis"), ',')) basis.push_back(std::atoi(s.c_str()));
    std::vector<double> cells, costs;
    for (const std::string &s : split(field("cells"), ',')) cells.push_back(from_hex(s));
    for (const std::string &s : split(field("costs"), ',')) costs.push_back(from_hex(s));
    const int m = (int)basis.size(), n = (int)num("n"), col = (int)num("col");
    if ((int)cells.size() != m || (int)costs.size() != n + 1 || col < 0 || col > n) return 2;
    const double acc = plan_cost_cell(
        col, m, n, [&](int r) { return basis[(size_t)r]; }, [&](int r) { return cells[(size_t)r]; },
        [&](int k) { return costs[(size_t)k]; });
    std::printf("acc=%016llx\n", (unsigned long long)bits_of(acc));
    return 0;
}

int sweep()
{
    const bool uniform = num("uniform") != 0;
    std::vector<int64_t> m, n;
    if (!shapes(m, n, uniform)) return 2;
    const int64_t count = (int64_t)m.size();
    std::vector<int64_t> toff((size_t)count + 1), boff((size_t)count + 1), coff((size_t)count + 1);
    for (int64_t i = 0; i < count; ++i) {
        const size_t u = (size_t)i;
        toff[u + 1] = toff[u] + (m[u] + 1) * (n[u] + 1);
        boff[u + 1] = boff[u] + m[u];
        coff[u + 1] = coff[u] + n[u];
    }
    const int64_t first = num("first"), cnt = num("count");
    if (first < 0 || cnt < 1 || first + cnt > count) return 2;
    // the whole batch's tableaux and bases, and the window's packed costs
    std::vector<double> T((size_t)toff[(size_t)count]);
    std::vector<int32_t> basis((size_t)boff[(size_t)count]);
    for (int64_t i = 0; i < count; ++i) {
        for (int64_t e = 0; e < toff[(size_t)i + 1] - toff[(size_t)i]; ++e)
            T[(size_t)(toff[(size_t)i] + e)] = cell_value(i, e);
        for (int64_t r = 0; r < m[(size_t)i]; ++r) {
            const int64_t k = (7 * r + 3 * i) % n[(size_t)i];
            basis[(size_t)(boff[(size_t)i] + r)] = (int32_t)(r % 3 == 1 ? (r % 2 ? -1 : n[(size_t)i]) : k);
        }
    }
    const int64_t pairs = coff[(size_t)(first + cnt)] - coff[(size_t)first] + cnt;
    std::vector<double> costs((size_t)pairs);
    for (int64_t k = 0; k < pairs; ++k) costs[(size_t)k] = cell_value(first + 5, 3 * k + 1);
    // the loop written out
    std::vector<double> want = T;
    for (int64_t i = first; i < first + cnt; ++i) {
        const size_t u = (size_t)i;
        const int64_t w = n[u] + 1, base = coff[u] - coff[(size_t)first] + (i - first);
        for (int64_t j = 0; j < w; ++j) {
            double acc = costs[(size_t)(base + j)];
            for (int64_t r = 0; r < m[u]; ++r) {
                const int64_t k = basis[(size_t)(boff[u] + r)];
                if (k < 0 || k >= n[u]) continue;
                const double p = costs[(size_t)(base + 1 + k)] * T[(size_t)(toff[u] + (1 + r) * w + j)];
                acc = acc - p;
            }
            want[(size_t)(toff[u] + j)] = acc;
        }
    }
    // every lane of the launch
    const FlatGrid g = plan_cost_grid(pairs);
    std::vector<double> got = T;
    std::vector<int> hits((size_t)(coff[(size_t)count] + count), 0);
    long long bad_map = 0;
    for (int64_t lane = 0; lane < g.blocks * g.threads; ++lane) {
        if (lane >= pairs) continue;            // the kernel's bound
        const CostAt at = uniform ? plan_cost_at(first, lane, (int)n[0])
                                  : plan_cost_at(first, first + cnt, lane, [&](long long i) {
                                        return (long long)(coff[(size_t)i] - coff[(size_t)first] + (i - first));
                                    });
        if (at.lp < first || at.lp >= first + cnt || at.col < 0 || at.col > n[(size_t)at.lp] ||
            at.base != coff[(size_t)at.lp] - coff[(size_t)first] + (at.lp - first)) {
            ++bad_map;
            continue;
        }
        const size_t u = (size_t)at.lp;
        ++hits[(size_t)(coff[u] + at.lp + at.col)];
        const int64_t w = n[u] + 1;
        const double *col = T.data() + toff[u] + w + at.col;
        const int32_t *bs = basis.data() + boff[u];
        const double *c = costs.data() + at.base;
        got[(size_t)(toff[u] + at.col)] = plan_cost_cell(
            at.col, (int)m[u], (int)n[u], [&](int r) { return (int)bs[r]; }, [&](int r) { return col[(int64_t)r * w]; },
            [&](int k) { return c[k]; });
    }
    long long bad_cells = 0, bad_rest = 0;
    for (int64_t i = 0; i < count; ++i) {
        const size_t u = (size_t)i;
        const bool in = i >= first && i < first + cnt;
        for (int64_t col = 0; col <= n[u]; ++col)
            if (hits[(size_t)(coff[u] + i + col)] != (in ? 1 : 0)) ++bad_map;
        for (int64_t row = 0; row <= m[u]; ++row)
            for (int64_t col = 0; col <= n[u]; ++col) {
                const size_t e = (size_t)(toff[u] + row * (n[u] + 1) + col);
                const bool same = bits_of(got[e]) == bits_of(want[e]);
                if (in && row == 0) bad_cells += same ? 0 : 1;
                else bad_rest += same && bits_of(got[e]) == bits_of(T[e]) ? 0 : 1;
            }
    }
    std::printf("pairs=%lld bad_map=%lld bad_cells=%lld bad_rest=%lld\n", (long long)pairs, bad_map, bad_cells,
                bad_rest);
    return 0;
}

int restage()
{
    const bool uniform = num("uniform") != 0;
    std::vector<int64_t> m, ns;
    if (!shapes(m, ns, uniform)) return 2;
    const int64_t count = (int64_t)m.size();
    std::vector<int64_t> poff((size_t)count + 1), voff((size_t)count + 1), yoff((size_t)count + 1);
    for (int64_t i = 0; i < count; ++i) {
        const size_t u = (size_t)i;
        poff[u + 1] = poff[u] + plan_general_block(m[u], ns[u]);
        voff[u + 1] = voff[u] + ns[u];
        yoff[u + 1] = yoff[u] + m[u];
    }
    const int64_t first = num("first"), cnt = num("count");
    if (first < 0 || cnt < 1 || first + cnt > count) return 2;
    auto start = [&](long long i) { return (long long)(3 * voff[(size_t)i] + yoff[(size_t)i] + i); };
    const int64_t lanes = start(first + cnt) - start(first);
    std::vector<double> stage((size_t)poff[(size_t)count]), border((size_t)lanes);
    for (size_t e = 0; e < stage.size(); ++e) stage[e] = cell_value(1, (int64_t)e);
    for (int64_t k = 0; k < lanes; ++k) border[(size_t)k] = 1000.0 + (double)k;
    // the border written out: where each of an LP's values belongs
    std::vector<double> want = stage;
    std::vector<int> is_border(stage.size(), 0);
    for (int64_t i = first; i < first + cnt; ++i) {
        const size_t u = (size_t)i;
        const double *src = border.data() + (start(i) - start(first));
        double *blk = want.data() + poff[u];
        int *mark = is_border.data() + poff[u];
        int64_t k = 0;
        for (int64_t j = 0; j <= ns[u]; ++j, ++k) blk[j] = src[k], mark[j] = 1;
        for (int64_t r = 0; r < m[u]; ++r, ++k) blk[(1 + r) * (ns[u] + 1)] = src[k], mark[(1 + r) * (ns[u] + 1)] = 1;
        for (int64_t j = 0; j < 2 * ns[u]; ++j, ++k)
            blk[(m[u] + 1) * (ns[u] + 1) + j] = src[k], mark[(m[u] + 1) * (ns[u] + 1) + j] = 1;
        if (k != plan_restage_border(m[u], ns[u])) return 2;
    }
    const FlatGrid g = plan_restage_grid(lanes);
    std::vector<double> got = stage;
    std::vector<int> hits(stage.size(), 0);
    long long bad_map = 0;
    for (int64_t lane = 0; lane < g.blocks * g.threads; ++lane) {
        if (lane >= lanes) continue;            // the kernel's bound
        long long e = -1;
        const long long lp = uniform ? plan_general_lane_lp<false>(first, cnt, lane, plan_restage_border(m[0], ns[0]),
                                                                   start, &e)
                                     : plan_general_lane_lp<true>(first, cnt, lane, 0, start, &e);
        if (lp < first || lp >= first + cnt || e < 0 || e >= plan_restage_border(m[(size_t)lp], ns[(size_t)lp])) {
            ++bad_map;
            continue;
        }
        const long long at = plan_restage_at(e, m[(size_t)lp], ns[(size_t)lp]);
        if (at < 0 || at >= plan_general_block(m[(size_t)lp], ns[(size_t)lp])) {
            ++bad_map;
            continue;
        }
        ++hits[(size_t)(poff[(size_t)lp] + at)];
        got[(size_t)(poff[(size_t)lp] + at)] = border[(size_t)lane];
    }
    long long bad_cells = 0, bad_rest = 0;
    for (size_t e = 0; e < stage.size(); ++e) {
        if (hits[e] != is_border[e]) ++bad_map;
        const bool same = bits_of(got[e]) == bits_of(want[e]);
        if (is_border[e]) bad_cells += same ? 0 : 1;
        else bad_rest += same ? 0 : 1;
    }
    std::printf("lanes=%lld bad_map=%lld bad_cells=%lld bad_rest=%lld\n", (long long)lanes, bad_map, bad_cells,
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
                std::fprintf(stderr, "batch_reopt_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        int st = 0;
        if (what == "grid") {
            const FlatGrid g = plan_cost_grid(num("pairs"));
            std::printf("blocks=%lld threads=%d\n", (long long)g.blocks, g.threads);
        } else if (what == "cell") {
            st = cell();
        } else if (what == "sweep") {
            st = sweep();
        } else if (what == "restage") {
            st = restage();
        } else {
            std::fprintf(stderr, "batch_reopt_check: request %s\n", what.c_str());
            return 2;
        }
        if (st) {
            std::fprintf(stderr, "batch_reopt_check: bad %s request\n", what.c_str());
            return st;
        }
    }
    return 0;
}
