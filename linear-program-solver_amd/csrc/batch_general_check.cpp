// Host-only driver of the general-form batches' rules (batch_plan.h:
// plan_general_counts, plan_general_tables, plan_general_shift,
// plan_general_cell, plan_general_lane, plan_general_lane_lp and the recovery
// formulas) for tests/test_batch_general_cpu.py: one request per line on stdin,
// one answer per line on stdout.
//
//   counts senses=012 kinds=01234 [m= ns=]
//       -> st= bad= m= ns= nf= nb= k= rows= cols= untouched=
//          st < 0: refused (-1 bad sense, -2 bad kind, with bad= the entry; -3
//          bad shape) and the output left alone (untouched=1)
//   tables senses=012 kinds=01234
//       -> st= var=src:brow:neg:kind,... slack=a,b,... bvar=a,b,...
//   grid lanes=
//       -> blocks= threads=          (blocks = -1: more than a grid holds)
//   sweep shapes=m:ns,m:ns,... senses=01/2/... kinds=04/2/... max=01... first= count= uniform=0|1
//       -> elems= shift_lanes= bad_shift= bad_map= bad_cells= bad_recover= bad_duals=
//          the batch's tables are derived as lp_general_set_form derives them and
//          every lane of the window's four launches is walked: bad_shift counts
//          entries of the shifted columns not written exactly once or not the
//          bits of a plain loop over the LP's variables; bad_map destination
//          elements not written exactly once or from another (kind, source)
//          than a plain walk over the LPs, rows and columns gives; bad_cells
//          the 64-bit cells in which the tableaux assembled through the lanes
//          differ from the formula written out; bad_recover and bad_duals the
//          caller variables (and objectives) and rows whose lane found another
//          LP or entry than the plain walk.  uniform=1: one shape and form, the
//          divisions of a uniform batch.
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
        std::fprintf(stderr, "batch_general_check: field %s missing\n", name);
        std::exit(2);
    }
    return it->second;
}
bool has(const char *name) { return g_fields.count(name) != 0; }
long long num(const char *name) { return std::atoll(field(name).c_str()); }

std::vector<int8_t> codes_of(const std::string &digits)
{
    std::vector<int8_t> s;
    for (char c : digits) s.push_back((int8_t)(c - '0'));
    return s;
}

std::vector<std::vector<int8_t>> lists_of(const std::string &text)
{
    std::vector<std::vector<int8_t>> out;
    std::istringstream ss(text);
    std::string one;
    while (std::getline(ss, one, '/')) out.push_back(codes_of(one));
    return out;
}

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

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
    std::vector<int64_t> m, ns;
    std::istringstream sh(field("shapes"));
    std::string one;
    while (std::getline(sh, one, ',')) {
        const size_t c = one.find(':');
        if (c == std::string::npos) return 2;
        m.push_back(std::atoll(one.substr(0, c).c_str()));
        ns.push_back(std::atoll(one.substr(c + 1).c_str()));
    }
    const std::vector<std::vector<int8_t>> sense = lists_of(field("senses")), kind = lists_of(field("kinds"));
    const std::vector<int8_t> maxi = codes_of(field("max"));
    const int64_t count = (int64_t)m.size();
    const bool uniform = num("uniform") != 0;
    if (sense.size() != (size_t)count || kind.size() != (size_t)count || maxi.size() != (size_t)count) return 2;
    // the batch's tables, as lp_general_set_form derives them
    const size_t C = (size_t)count;
    std::vector<GeneralCounts> cnt(C);
    std::vector<int64_t> toff(C + 1), boff(C + 1), coff(C + 1), poff(C + 1), xoff(C + 1), voff(C + 1), yoff(C + 1);
    std::vector<GVar> var;
    std::vector<int32_t> slack, bvar;
    for (size_t i = 0; i < C; ++i) {
        if ((int64_t)sense[i].size() != m[i] || (int64_t)kind[i].size() != ns[i]) return 2;
        if (uniform && (m[i] != m[0] || ns[i] != ns[0] || sense[i] != sense[0] || kind[i] != kind[0] || maxi[i] != maxi[0]))
            return 2;
        if (plan_general_counts(sense[i].data(), kind[i].data(), m[i], ns[i], &cnt[i]) != 0) return 2;
        const GeneralCounts &c = cnt[i];
        if (!uniform || i == 0) {
            const size_t x0 = var.size(), s0 = slack.size();
            var.resize(x0 + (size_t)(c.ns + c.nf));
            slack.resize(s0 + (size_t)c.rows);
            bvar.resize(s0 + (size_t)c.rows);
            if (plan_general_tables(sense[i].data(), kind[i].data(), m[i], ns[i], var.data() + x0, slack.data() + s0,
                                    bvar.data() + s0) != 0)
                return 2;
        }
        toff[i + 1] = toff[i] + (c.rows + 1) * (c.cols + 1);
        boff[i + 1] = boff[i] + c.rows;
        coff[i + 1] = coff[i] + c.cols;
        poff[i + 1] = poff[i] + plan_general_block(c.m, c.ns);
        xoff[i + 1] = uniform ? 0 : xoff[i] + c.ns + c.nf;
        voff[i + 1] = voff[i] + c.ns;
        yoff[i + 1] = yoff[i] + c.m;
    }
    auto shape = [&](long long i) {
        const GeneralCounts &c = cnt[(size_t)i];
        return GeneralLp{toff[(size_t)i], boff[(size_t)i], coff[(size_t)i], poff[(size_t)i], xoff[(size_t)i],
                         uniform ? 0 : boff[(size_t)i], voff[(size_t)i], yoff[(size_t)i], (int)c.m, (int)c.rows,
                         (int)c.cols, (int)c.ns, (int)c.nf, (int)maxi[(size_t)i]};
    };
    const int64_t first = num("first"), win = num("count");
    if (first < 0 || win < 1 || first + win > count) return 2;
    const size_t lo = (size_t)first, hi = (size_t)(first + win);
    const int64_t tbase = toff[lo], elems = toff[hi] - tbase;

    // the staged blocks of the whole batch (only the window's are read) and the formula written out
    std::vector<double> stage((size_t)poff[C]);
    for (size_t i = 0; i < C; ++i)
        for (int64_t k = 0; k < poff[i + 1] - poff[i]; ++k) stage[(size_t)(poff[i] + k)] = staged_value((int64_t)i, k);
    std::vector<double> want((size_t)elems, 0.0), want_shift((size_t)(boff[C] + count), -7.0);
    for (size_t i = lo; i < hi; ++i) {
        const GeneralCounts &c = cnt[i];
        const bool mx = maxi[i] != 0;
        const int64_t w = c.cols + 1, pw = c.ns + 1;
        double *T = want.data() + (toff[i] - tbase);
        const double *P = stage.data() + poff[i], *lb = P + (c.m + 1) * pw, *ub = lb + c.ns;
        int64_t f = 0, t = 0, sl = 0;
        for (int64_t row = 0; row <= c.m; ++row) {
            double acc = row == 0 && mx ? plan_flip(P[0]) : P[row * pw];
            for (int64_t j = 0; j < c.ns; ++j) {
                const int kj = kind[i][(size_t)j];
                if (kj != PLAN_VAR_LOWER && kj != PLAN_VAR_BOXED && kj != PLAN_VAR_UPPER) continue;
                const double a = row == 0 && mx ? plan_flip(P[1 + j]) : P[row * pw + 1 + j];
                const double prod = a * (kj == PLAN_VAR_UPPER ? ub[j] : lb[j]);
                acc = acc - prod;
            }
            T[row * w] = acc;
            want_shift[(size_t)(boff[i] + (int64_t)i + row)] = acc;
        }
        for (int64_t j = 0; j < c.ns; ++j) {
            const int kj = kind[i][(size_t)j];
            const bool up = kj == PLAN_VAR_UPPER;
            for (int64_t row = 0; row <= c.m; ++row) {
                const double v = P[row * pw + 1 + j];
                const bool flip = row == 0 ? mx != up : up;
                T[row * w + 1 + j] = flip ? plan_flip(v) : v;
                if (kj == PLAN_VAR_FREE) T[row * w + 1 + c.ns + f] = plan_flip(T[row * w + 1 + j]);
            }
            if (kj == PLAN_VAR_FREE) ++f;
            if (kj == PLAN_VAR_BOXED) {
                const int64_t row = 1 + c.m + t;
                T[row * w] = ub[j] - lb[j];
                want_shift[(size_t)(boff[i] + (int64_t)i + row)] = T[row * w];
                T[row * w + 1 + j] = 1.0;
                T[row * w + 1 + c.ns + c.nf + c.k + t] = 1.0;
                ++t;
            }
        }
        for (int64_t row = 1; row <= c.m; ++row) {
            const int s = sense[i][(size_t)(row - 1)];
            if (s == PLAN_SENSE_EQ) continue;
            T[row * w + 1 + c.ns + c.nf + sl] = s == PLAN_SENSE_LE ? 1.0 : -1.0;
            ++sl;
        }
    }

    // launch 1: the shifted columns
    const int64_t shift_lanes = boff[hi] - boff[lo] + win;
    std::vector<double> shift((size_t)(boff[C] + count), -7.0);
    std::vector<int> shits(shift.size(), 0);
    long long bad_shift = 0;
    const FlatGrid sg = plan_general_grid(shift_lanes);
    for (int64_t g = 0; g < sg.blocks * sg.threads; ++g) {
        if (g >= shift_lanes) continue;
        long long row = -1;
        auto start = [&](long long i) { return (long long)(boff[(size_t)i] + i); };
        const long long lp = uniform ? plan_general_lane_lp<false>(first, win, g, cnt[0].rows + 1, start, &row)
                                     : plan_general_lane_lp<true>(first, win, g, 0, start, &row);
        if (lp < first || lp >= first + win || row < 0 || row > cnt[(size_t)lp].rows) {
            ++bad_shift;
            continue;
        }
        const GeneralLp L = shape(lp);
        const GVar *v = var.data() + L.xoff;
        const int bv = row > L.m ? bvar[(size_t)(L.soff + row - 1)] : 0;
        const size_t at = (size_t)(L.boff + lp + row);
        ++shits[at];
        shift[at] = plan_general_shift((int)row, L.m, L.ns, L.maximise != 0, stage.data() + L.poff,
                                       [&](int j) { return v[j]; }, bv);
    }
    for (size_t i = lo; i < hi; ++i)
        for (int64_t row = 0; row <= cnt[i].rows; ++row) {
            const size_t at = (size_t)(boff[i] + (int64_t)i + row);
            if (shits[at] != 1 || !same(shift[at], want_shift[at])) ++bad_shift;
        }
    for (size_t at = 0; at < shits.size(); ++at)
        if (shits[at] != 0 && (at < (size_t)(boff[lo] + first) || at >= (size_t)(boff[hi] + first + win))) ++bad_shift;

    // launch 2: every lane of the assembly
    const FlatGrid g = plan_general_grid(elems);
    std::vector<double> got((size_t)elems, -7.0);
    std::vector<int> hits((size_t)elems, 0);
    long long bad_map = 0;
    const int64_t E0 = (cnt[0].rows + 1) * (cnt[0].cols + 1);
    auto kind_of = [&](size_t i, int64_t j) { return (int)kind[i][(size_t)j]; };
    // the sense of tableau row `row` >= 1: a bound row is a <= row
    auto sense_of = [&](size_t i, int64_t row) {
        return row <= cnt[i].m ? (int)sense[i][(size_t)(row - 1)] : PLAN_SENSE_LE;
    };
    auto put = [&](long long e, int kind, long long at) {
        if (e < 0 || e >= elems) {
            ++bad_map;
            return;
        }
        ++hits[(size_t)e];
        // the plain walk's (kind, source) of this element
        size_t i = lo;
        while (i + 1 < hi && toff[i + 1] - tbase <= e) ++i;
        const GeneralCounts &c = cnt[i];
        const int64_t w = c.cols + 1, rem = e - (toff[i] - tbase), row = rem / w, col = rem % w;
        int wkind = PLAN_CELL_ZERO;
        long long wsrc = -1;
        if (col == 0) {
            wkind = row <= c.m ? PLAN_CELL_SHIFTED : PLAN_CELL_RANGE;
            wsrc = boff[i] + (int64_t)i + row;
        } else if (col <= c.ns + c.nf) {
            int64_t j = col - 1;
            bool negpart = false;
            if (col > c.ns) {           // the (col - ns)-th FREE variable
                int64_t f = col - c.ns;
                for (j = 0; j < c.ns; ++j)
                    if (kind_of(i, j) == PLAN_VAR_FREE && --f == 0) break;
                negpart = true;
            }
            const int kj = kind_of(i, j);
            if (row <= c.m) {
                const bool fl = negpart || kj == PLAN_VAR_UPPER;
                const bool flip = row == 0 ? (maxi[i] != 0) != fl : fl;
                wkind = flip ? PLAN_CELL_STAGED_FLIP : PLAN_CELL_STAGED;
                wsrc = poff[i] + row * (c.ns + 1) + 1 + j;
            } else if (!negpart && kj == PLAN_VAR_BOXED) {
                int64_t t = 0;
                for (int64_t q = 0; q < j; ++q) t += kind_of(i, q) == PLAN_VAR_BOXED ? 1 : 0;
                wkind = row == 1 + c.m + t ? PLAN_CELL_PLUS : PLAN_CELL_ZERO;
            }
        } else if (row >= 1) {
            int64_t t = 0;              // the non-equality rows before this one
            for (int64_t q = 1; q < row; ++q) t += sense_of(i, q) != PLAN_SENSE_EQ ? 1 : 0;
            const int s = sense_of(i, row);
            if (s != PLAN_SENSE_EQ && col == 1 + c.ns + c.nf + t)
                wkind = s == PLAN_SENSE_LE ? PLAN_CELL_PLUS : PLAN_CELL_MINUS;
        }
        if (kind != wkind || at != wsrc) ++bad_map;
        got[(size_t)e] = kind == PLAN_CELL_STAGED        ? stage[(size_t)at]
                         : kind == PLAN_CELL_STAGED_FLIP ? plan_flip(stage[(size_t)at])
                         : kind == PLAN_CELL_SHIFTED || kind == PLAN_CELL_RANGE ? shift[(size_t)at]
                         : kind == PLAN_CELL_PLUS  ? 1.0
                         : kind == PLAN_CELL_MINUS ? -1.0
                                                   : 0.0;
    };
    auto var_at = [&](long long at) { return var[(size_t)at]; };
    auto slack_at = [&](long long at) { return (int)slack[(size_t)at]; };
    for (int64_t lane = 0; lane < g.blocks * g.threads; ++lane) {
        if (uniform)
            plan_general_lane(lane, elems, tbase, [&](long long e) { return first + e / E0; }, shape, var_at, slack_at,
                              put);
        else
            plan_general_lane(
                lane, elems, tbase,
                [&](long long e) {
                    return plan_lane_lp(first, first + win, e, [&](long long i) { return (long long)(toff[(size_t)i] - tbase); });
                },
                shape, var_at, slack_at, put);
    }
    long long bad_cells = 0;
    for (int64_t e = 0; e < elems; ++e) {
        if (hits[(size_t)e] != 1) ++bad_map;
        if (!same(got[(size_t)e], want[(size_t)e])) ++bad_cells;
    }

    // launches 3 and 4: the lanes of the recovery and of the duals find their LP and entry
    long long bad_recover = 0, bad_duals = 0;
    {
        const int64_t lanes = voff[hi] - voff[lo] + win;
        std::vector<int> seen((size_t)lanes, 0);
        auto start = [&](long long i) { return (long long)(voff[(size_t)i] + i); };
        for (int64_t q = 0; q < lanes; ++q) {
            long long j = -1;
            const long long lp = uniform ? plan_general_lane_lp<false>(first, win, q, cnt[0].ns + 1, start, &j)
                                         : plan_general_lane_lp<true>(first, win, q, 0, start, &j);
            if (lp < first || lp >= first + win || j < 0 || j > cnt[(size_t)lp].ns) {
                ++bad_recover;
                continue;
            }
            ++seen[(size_t)(voff[(size_t)lp] - voff[lo] + (lp - first) + j)];
        }
        for (int v : seen) bad_recover += v != 1 ? 1 : 0;
    }
    {
        const int64_t rows = yoff[hi] - yoff[lo], vars = voff[hi] - voff[lo];
        std::vector<int> seen((size_t)(rows + vars), 0);
        for (int64_t q = 0; q < rows + vars; ++q) {
            const bool isrow = q < rows;
            const std::vector<int64_t> &off = isrow ? yoff : voff;
            auto start = [&](long long i) { return (long long)off[(size_t)i]; };
            const int64_t stride = isrow ? cnt[0].m : cnt[0].ns, qq = isrow ? q : q - rows;
            long long at = -1;
            const long long lp = uniform ? plan_general_lane_lp<false>(first, win, qq, stride, start, &at)
                                         : plan_general_lane_lp<true>(first, win, qq, 0, start, &at);
            const int64_t size = lp < first || lp >= first + win ? -1 : isrow ? cnt[(size_t)lp].m : cnt[(size_t)lp].ns;
            if (at < 0 || at >= size) {
                ++bad_duals;
                continue;
            }
            ++seen[(size_t)((isrow ? 0 : rows) + off[(size_t)lp] - off[lo] + at)];
        }
        for (int v : seen) bad_duals += v != 1 ? 1 : 0;
    }
    std::printf("elems=%lld shift_lanes=%lld bad_shift=%lld bad_map=%lld bad_cells=%lld bad_recover=%lld bad_duals=%lld\n",
                (long long)elems, (long long)shift_lanes, bad_shift, bad_map, bad_cells, bad_recover, bad_duals);
    return 0;
}

std::string join(const std::vector<int32_t> &v)
{
    std::string t;
    for (size_t r = 0; r < v.size(); ++r) t += (r ? "," : "") + std::to_string(v[r]);
    return t.empty() ? "-" : t;
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
                std::fprintf(stderr, "batch_general_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "counts") {
            const std::vector<int8_t> s = codes_of(field("senses")), k = codes_of(field("kinds"));
            const int64_t m = has("m") ? num("m") : (int64_t)s.size(), ns = has("ns") ? num("ns") : (int64_t)k.size();
            GeneralCounts c;
            c.m = c.ns = c.nf = c.nb = c.k = c.rows = c.cols = -5;
            int64_t bad = -1;
            const int64_t st = plan_general_counts(s.empty() ? nullptr : s.data(), k.empty() ? nullptr : k.data(), m, ns,
                                                   &c, &bad);
            const bool untouched = c.m == -5 && c.ns == -5 && c.nf == -5 && c.nb == -5 && c.k == -5 && c.rows == -5 &&
                                   c.cols == -5;
            std::printf("st=%lld bad=%lld m=%lld ns=%lld nf=%lld nb=%lld k=%lld rows=%lld cols=%lld untouched=%d\n",
                        (long long)st, (long long)bad, (long long)c.m, (long long)c.ns, (long long)c.nf,
                        (long long)c.nb, (long long)c.k, (long long)c.rows, (long long)c.cols, untouched ? 1 : 0);
        } else if (what == "tables") {
            const std::vector<int8_t> s = codes_of(field("senses")), k = codes_of(field("kinds"));
            GeneralCounts c;
            int64_t st = plan_general_counts(s.data(), k.data(), (int64_t)s.size(), (int64_t)k.size(), &c);
            if (st != 0) {
                std::printf("st=%lld var=- slack=- bvar=-\n", (long long)st);
                continue;
            }
            std::vector<GVar> var((size_t)(c.ns + c.nf));
            std::vector<int32_t> slack((size_t)c.rows), bvar((size_t)c.rows);
            st = plan_general_tables(s.data(), k.data(), c.m, c.ns, var.data(), slack.data(), bvar.data());
            std::string v;
            for (size_t j = 0; j < var.size(); ++j)
                v += (j ? "," : "") + std::to_string(var[j].src) + ":" + std::to_string(var[j].brow) + ":" +
                     std::to_string(var[j].neg) + ":" + std::to_string(var[j].kind);
            std::printf("st=%lld var=%s slack=%s bvar=%s\n", (long long)st, v.c_str(), join(slack).c_str(),
                        join(bvar).c_str());
        } else if (what == "grid") {
            const FlatGrid g = plan_general_grid(num("lanes"));
            std::printf("blocks=%lld threads=%d\n", (long long)g.blocks, g.threads);
        } else if (what == "sweep") {
            const int st = sweep();
            if (st) {
                std::fprintf(stderr, "batch_general_check: bad sweep request\n");
                return st;
            }
        } else {
            std::fprintf(stderr, "batch_general_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
