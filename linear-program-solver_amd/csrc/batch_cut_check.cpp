// Host-only driver of the warm cuts' rules (batch_plan.h: CutLp, plan_cut_next,
// plan_cut_cell, plan_cut_lane, plan_cut_at, plan_cut_rows) for
// tests/test_batch_cut_cpu.py: one request per line on stdin, one answer per
// line on stdout.
//
//   knobs
//       -> group= run= threads=
//   walk shapes=m:n:q,m:n:q,... first= count=
//       -> elems= lanes= nbasis= cells=tok,tok,... basis=tok,tok,... bad=
//          The table of the window is built as lp_cut_extend builds it, both
//          batches packed LP after LP, and every lane of the three launches is
//          walked with the kernels' own lookups.  cells has one token per
//          element of the whole destination batch: c<k> a copy of element k of
//          the whole source batch, z +0.0, o +1.0, p a cell k_cut_rows' lanes
//          wrote, - untouched.  basis likewise per destination basis entry:
//          s<k> the source's entry k, n<v> the value v, - untouched.  bad
//          counts cells or entries written more than once, lanes that fall
//          outside the window, and priced cells k_cut_copy did not skip.
//   rows g= n= basis=a,b,... cells=hex,... rows=hex,... sense=0,1,...
//       -> priced=hex,hex,...
//          the q x (n+1) priced cells, q = len(sense), of one LP whose stored
//          rows 1..m are `cells` (m x (n+1), row-major), computed in groups of
//          g new rows: g = 1, g = the build's PLAN_CUT_GROUP, or g = 0 for the
//          kernel's own lane map (plan_cut_lanes, plan_cut_at).
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
        std::fprintf(stderr, "batch_cut_check: field %s missing\n", name);
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

void print_list(const char *name, const std::vector<std::string> &toks)
{
    std::printf("%s=", name);
    for (size_t i = 0; i < toks.size(); ++i) std::printf("%s%s", i ? "," : "", toks[i].c_str());
}

int walk()
{
    std::vector<int64_t> m, n, q;
    for (const std::string &one : split(field("shapes"), ',')) {
        const std::vector<std::string> p = split(one, ':');
        if (p.size() != 3) return 2;
        m.push_back(std::atoll(p[0].c_str()));
        n.push_back(std::atoll(p[1].c_str()));
        q.push_back(std::atoll(p[2].c_str()));
        if (m.back() < 1 || n.back() < 1 || q.back() < 0) return 2;
    }
    const int64_t all = (int64_t)m.size(), first = num("first"), count = num("count");
    if (first < 0 || count < 1 || first + count > all) return 2;
    std::vector<int64_t> stoff((size_t)all + 1), dtoff((size_t)all + 1), sboff((size_t)all + 1), dboff((size_t)all + 1);
    for (int64_t i = 0; i < all; ++i) {
        const size_t u = (size_t)i;
        stoff[u + 1] = stoff[u] + (m[u] + 1) * (n[u] + 1);
        dtoff[u + 1] = dtoff[u] + (m[u] + q[u] + 1) * (n[u] + q[u] + 1);
        sboff[u + 1] = sboff[u] + m[u];
        dboff[u + 1] = dboff[u] + m[u] + q[u];
    }
    // the table, as lp_cut_extend builds it
    std::vector<CutLp> tab((size_t)count + 1);
    CutLp at{};
    for (int64_t k = 0; k < count; ++k) {
        const size_t u = (size_t)(first + k);
        at.stoff = stoff[u];
        at.dtoff = dtoff[u];
        at.sboff = sboff[u];
        at.dboff = dboff[u];
        at.m = (int32_t)m[u];
        at.n = (int32_t)n[u];
        at.q = (int32_t)q[u];
        tab[(size_t)k] = at;
        at = plan_cut_next(at);
    }
    tab[(size_t)count] = at;
    const int64_t elems = at.e0, nbasis = at.b0, lanes = at.lane0;
    std::vector<std::string> cells((size_t)dtoff[(size_t)all], "-"), basis((size_t)dboff[(size_t)all], "-");
    long long bad = 0;
    auto put_cell = [&](long long to, const std::string &tok) {
        if (to < 0 || to >= (long long)cells.size() || cells[(size_t)to] != "-") ++bad;
        else cells[(size_t)to] = tok;
    };
    const CutLp *lp = tab.data();
    // k_cut_copy
    const FlatGrid cg = plan_cut_copy_grid(elems);
    for (int64_t g = 0; g < cg.blocks * cg.threads; ++g)
        plan_cut_lane(
            g * PLAN_ASSEMBLE_RUN, elems,
            [&](long long e) { return plan_lane_lp(0, count, e, [&](long long k) { return lp[k].e0; }); },
            [&](long long k) {
                if (k < 0 || k >= count) ++bad, k = 0;
                return lp[k];
            },
            [&](long long to, int kind, long long from) {
                if (kind == PLAN_CUT_PRICED) return;
                if (kind == PLAN_CUT_COPY && (from < 0 || from >= stoff[(size_t)all])) ++bad;
                put_cell(to, kind == PLAN_CUT_COPY ? "c" + std::to_string(from) : kind == PLAN_CUT_ONE ? "o" : "z");
            });
    // k_cut_rows: which cells its lanes write
    const FlatGrid rg = plan_cut_grid(lanes);
    for (int64_t g = 0; g < rg.blocks * rg.threads; ++g) {
        if (g >= lanes) continue;           // the kernel's bound
        const long long k = plan_lane_lp(0, count, g, [&](long long i) { return lp[i].lane0; });
        const CutLp L = lp[k];
        if (g < L.lane0 || g >= L.lane0 + plan_cut_lanes(L.n, L.q)) {
            ++bad;
            continue;
        }
        const CutAt c = plan_cut_at(g - L.lane0, L.n);
        const int k1 = std::min<int>(L.q, c.k0 + PLAN_CUT_GROUP);
        if (c.col < 0 || c.col > L.n || c.k0 < 0 || c.k0 >= L.q) ++bad;
        for (int kk = c.k0; kk < k1; ++kk)
            put_cell(L.dtoff + (long long)(1 + L.m + kk) * (L.n + L.q + 1) + c.col, "p");
    }
    // k_cut_basis
    const FlatGrid bg = plan_cut_grid(nbasis);
    for (int64_t g = 0; g < bg.blocks * bg.threads; ++g) {
        if (g >= nbasis) continue;
        const CutLp L = lp[plan_lane_lp(0, count, g, [&](long long i) { return lp[i].b0; })];
        const long long r = g - L.b0;
        if (r < 0 || r >= L.m + L.q || basis[(size_t)(L.dboff + r)] != "-") {
            ++bad;
            continue;
        }
        basis[(size_t)(L.dboff + r)] = r < L.m ? "s" + std::to_string(L.sboff + r) : "n" + std::to_string(L.n + (r - L.m));
    }
    std::printf("elems=%lld lanes=%lld nbasis=%lld ", (long long)elems, (long long)lanes, (long long)nbasis);
    print_list("cells", cells);
    std::printf(" ");
    print_list("basis", basis);
    std::printf(" bad=%lld\n", bad);
    return 0;
}

template <int G>
void priced_groups(int m, int n, int q, const std::vector<int> &basis, const std::vector<double> &cells,
                   const std::vector<double> &rows, std::vector<double> &out)
{
    const int w = n + 1;
    for (int k0 = 0; k0 < q; k0 += G)
        for (int j = 0; j <= n; ++j)
            plan_cut_rows<G>(
                j, m, n, k0, std::min(q, k0 + G), [&](int r) { return basis[(size_t)r]; },
                [&](int r) { return cells[(size_t)(r * w + j)]; }, [&](int k, int c) { return rows[(size_t)(k * w + c)]; },
                [&](int k, double acc) { out[(size_t)(k * w + j)] = acc; });
}

int rows()
{
    std::vector<int> basis, sense;
    for (const std::string &s : split(field("basis"), ',')) basis.push_back(std::atoi(s.c_str()));
    for (const std::string &s : split(field("sense"), ',')) sense.push_back(std::atoi(s.c_str()));
    std::vector<double> cells, rows;
    for (const std::string &s : split(field("cells"), ',')) cells.push_back(from_hex(s));
    for (const std::string &s : split(field("rows"), ',')) rows.push_back(from_hex(s));
    const int m = (int)basis.size(), n = (int)num("n"), q = (int)sense.size(), g = (int)num("g"), w = n + 1;
    if ((int)cells.size() != m * w || (int)rows.size() != q * w || q < 1) return 2;
    std::vector<double> out((size_t)(q * w), -1.0);
    if (g == 1) {
        priced_groups<1>(m, n, q, basis, cells, rows, out);
    } else if (g == PLAN_CUT_GROUP) {
        priced_groups<PLAN_CUT_GROUP>(m, n, q, basis, cells, rows, out);
    } else if (g == 0) {        // the kernel's lanes
        for (long long lane = 0; lane < plan_cut_lanes(n, q); ++lane) {
            const CutAt at = plan_cut_at(lane, n);
            plan_cut_rows<PLAN_CUT_GROUP>(
                at.col, m, n, at.k0, std::min(q, at.k0 + PLAN_CUT_GROUP), [&](int r) { return basis[(size_t)r]; },
                [&](int r) { return cells[(size_t)(r * w + at.col)]; },
                [&](int k, int c) { return rows[(size_t)(k * w + c)]; },
                [&](int k, double acc) { out[(size_t)(k * w + at.col)] = acc; });
        }
    } else {
        return 2;
    }
    std::printf("priced=");
    for (int k = 0; k < q; ++k)
        for (int j = 0; j < w; ++j) {
            const double v = out[(size_t)(k * w + j)];
            std::printf("%s%016llx", k + j ? "," : "",
                        (unsigned long long)bits_of(sense[(size_t)k] == PLAN_SENSE_GE ? plan_cut_flip(v) : v));
        }
    std::printf("\n");
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
                std::fprintf(stderr, "batch_cut_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        int st = 0;
        if (what == "knobs") {
            std::printf("group=%d run=%d threads=%d\n", PLAN_CUT_GROUP, PLAN_ASSEMBLE_RUN, PLAN_FLAT_THREADS);
        } else if (what == "walk") {
            st = walk();
        } else if (what == "rows") {
            st = rows();
        } else {
            std::fprintf(stderr, "batch_cut_check: request %s\n", what.c_str());
            return 2;
        }
        if (st) {
            std::fprintf(stderr, "batch_cut_check: bad %s request\n", what.c_str());
            return st;
        }
    }
    return 0;
}
