// Host-only driver of the launch planners (geometry.h) and the knob parser
// (knobs.h) for tests/test_geometry_cpu.py: one request per line on stdin,
// one answer per line on stdout, every field as key=value.
//
//   pitch n= raw=
//   sweep rows= n= ld= nd_max= cnt= share= second= cus= bpc= tail= split=
//   sel   rc= n= bmax= xcd_cus= xr= xs_ok= share= occ= k=
//   group rc= ld= n= bmax= xr= nshard= share= xs_ok= cus= hier= occ= k=
//   knobs NAME=VALUE ...
//
// occ: the model standing in for the runtime's occupancy answer -- const (k
// blocks per CU), lds (160 KiB / the block's LDS rounded up to 2 KiB, at most
// k), missing (no variant is compiled).  const and lds know the variants the
// library compiles and call every other one missing.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "geometry.h"
#include "knobs.h"

using namespace lpk;

namespace {

std::map<std::string, std::string> g_fields;

const char *lookup(const char *name)
{
    auto it = g_fields.find(name);
    return it == g_fields.end() ? nullptr : it->second.c_str();
}
long long num(const char *name)
{
    const char *v = lookup(name);
    if (!v) {
        std::fprintf(stderr, "geometry_check: field %s missing\n", name);
        std::exit(2);
    }
    return std::atoll(v);
}

bool compiled(const Variant &v)
{
    if (v.sel) return (v.ipl == 1 || v.ipl == 2 || v.ipl == 4) && (v.rpl == 64 || (v.rpl == 32 && !v.xs));
#define X(NRV, IPLV, RPLV) \
    if (v.nr == NRV && v.ipl == IPLV && v.rpl == RPLV) return true;
    GROUP_VARIANTS(X)
#undef X
    return false;
}

Occupancy model()
{
    const std::string occ = lookup("occ") ? lookup("occ") : "";
    const int k = (int)num("k");
    if (occ == "const") return [k](const Variant &v) { return compiled(v) ? k : OCC_MISSING; };
    if (occ == "lds")
        return [k](const Variant &v) {
            if (!compiled(v)) return OCC_MISSING;
            const long long per = ((long long)v.lds + 2047) / 2048 * 2048;
            return (int)std::min<long long>(k, 160 * 1024 / per);
        };
    if (occ == "missing") return [](const Variant &) { return OCC_MISSING; };
    std::fprintf(stderr, "geometry_check: occ=%s\n", occ.c_str());
    std::exit(2);
}

void print_geom(const GroupGeom &G)
{
    std::printf("g=%lld nr=%d ipl=%d rpl=%d xmode=%d hk=%d lds=%zu per_cu=%d sel=%d xs=%d\n", G.g, G.nr, G.ipl, G.rpl,
                G.xmode, G.hk, G.lds, G.per_cu, G.sel, G.xs);
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
                std::fprintf(stderr, "geometry_check: %s\n", kv.c_str());
                return 2;
            }
            g_fields[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        if (what == "pitch") {
            std::printf("ld=%lld\n", (long long)row_pitch(num("n"), num("raw") != 0));
        } else if (what == "sweep") {
            const SweepShape S{num("rows"), num("n"), num("ld"), (int)num("nd_max"), (int)num("cnt"),
                               (int)num("share"), num("second") != 0};
            const SweepEnv E{(int)num("cus"), (int)num("bpc"), (int)num("tail"), std::atof(lookup("split"))};
            const SweepPlan P = plan_sweep(S, E);
            std::printf("rl=%d W=%d D=%d oop=%d nb=%d nexp=%d zero=%d nsg=%lld nrun=%lld run=%lld runb=%lld na=%d "
                        "tail=%lld tcol=%lld tend=%lld grid=%lld\n",
                        P.k.rl, P.k.W, P.k.D, P.k.oop, P.k.nb, P.k.nexp, P.k.rl && P.k.nexp < P.k.nb, P.nsg, P.nrun,
                        P.run, P.runb, P.na, P.tail, P.tcol, P.tend, P.grid);
        } else if (what == "sel") {
            print_geom(plan_sel(num("rc"), num("n"), (int)num("bmax"), (int)num("xcd_cus"), num("xr") != 0,
                                num("xs_ok") != 0, (int)num("share"), model()));
        } else if (what == "group") {
            print_geom(plan_group(num("rc"), num("ld"), num("n"), (int)num("bmax"), (int)num("xr"),
                                  (int)num("nshard"), (int)num("share"), num("xs_ok") != 0, (int)num("cus"),
                                  (int)num("hier"), model()));
        } else if (what == "knobs") {
            const ProcessKnobs p = parse_process_knobs(lookup);
            const HandleKnobs h = parse_handle_knobs(lookup);
            std::printf("sweep_oop=%d oop_room_mb=%llu oop_fail_alloc=%d sweep_cus=%d sweep_tail=%d sweep_split=%.17g "
                        "coop=%d hier=%d gmaj=%d ld_raw=%d persistent=%d spin_max=%u xwait_ms=%u fault_launch=%d "
                        "fault_t=%d fault_xcc=%d strict=%d xs_ok=%d peer_enable=%d stamps=%d xr_xcd=%d\n",
                        p.sweep_oop, p.oop_room_mb, p.oop_fail_alloc, p.sweep_cus, p.sweep_tail, p.sweep_split, p.coop,
                        p.hier, p.gmaj, p.ld_raw, h.persistent, h.spin_max, h.xwait_ms, h.fault_launch, h.fault_t,
                        h.fault_xcc, h.strict, h.xs_ok, h.peer_enable, h.stamps, h.xr_xcd);
        } else {
            std::fprintf(stderr, "geometry_check: request %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
