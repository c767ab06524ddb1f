// Stand-alone driver of the record planner (nupgcm_amd/csrc/csr_records_core.h) for tests/test_records_plan.py: reads one case
// as raw little-endian arrays from a directory, plans, writes every array of the plan back.  No GPU, no HIP: built with g++ under
// AddressSanitizer and UBSan by the test.
//   records_plan_main DIR         DIR/meta.txt: "key value" lines; DIR/{rowptr.i64, col.i32, val.f64[, gn_col.i32, gn_ncomp.i32]}
#include <cstdio>
#include <fstream>
#include <map>
#include <string>

#include "../nupgcm_amd/csrc/csr_records_core.h"

using namespace npg;

static std::string dir;

template <class T>
static std::vector<T> load(const char *name) {
    std::ifstream f(dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!f) return {};
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}
template <class T>
static void save(const char *name, const std::vector<T> &v) {
    std::ofstream f(dir + "/out_" + name, std::ios::binary);
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
static void save_tiles(const char *name, const std::vector<PlanTile> &t) {
    std::vector<int64_t> v;
    for (const PlanTile &q : t)
        for (int64_t x : {q.base, q.pbase, (int64_t)q.r0, (int64_t)q.nrows, (int64_t)q.n, (int64_t)q.npe, (int64_t)q.woff, (int64_t)q.voff, (int64_t)q.nw, (int64_t)q.nv})
            v.push_back(x);
    save(name, v);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    dir = argv[1];
    std::map<std::string, double> meta;
    {
        std::ifstream f(dir + "/meta.txt");
        std::string k;
        double v;
        while (f >> k >> v) meta[k] = v;
    }
    const std::vector<int64_t> rowptr = load<int64_t>("rowptr.i64");
    const std::vector<int32_t> col = load<int32_t>("col.i32");
    const std::vector<double> val = load<double>("val.f64");
    const HostCsr A{(int64_t)meta["m"], (int64_t)meta["n"], rowptr.data(), col.data(), val.data()};
    const NodeOrder o{(int64_t)meta["nfull"], (int64_t)meta["nsurf"]};
    const RecordCaps caps;
    std::ofstream out(dir + "/out_meta.txt");
    if (meta["full"] != 0) {
        const PackPlan F = plan_full_records(A, o, caps.tile_slots);
        out << "outcome " << (int)F.outcome << "\n";
        save("prow.i64", F.prow);
        save("grow.i64", F.grow);
        save("drow.i64", F.drow);
        save("rowptr.i64", F.rowptr);
        save("pcol.i32", F.pcol);
        save("gcol.i32", F.gcol);
        save("dcol.i32", F.dcol);
        save("col.i32", F.col);
        save("map9.i64", F.map9);
        save("mapg.i64", F.mapg);
        save("mapd.i64", F.mapd);
        save("maprem.i64", F.maprem);
        return 0;
    }
    RecordSwitches sw;
    sw.window = meta["window"] != 0;
    sw.column_records = meta["column_records"] != 0;
    sw.coupling = meta["coupling"] != 0;
    sw.win_rows = meta["win_rows"] != 0;
    sw.win_bytes = (int64_t)meta["win_bytes"];
    sw.win_scale = meta["win_scale"];
    sw.win_order = (int)meta["win_order"];
    const RecordPlan P = plan_block_records(A, o, meta["rtol"], sw, caps.tile_slots);
    out << "outcome " << (int)P.outcome << "\npadded " << P.padded << "\ncolrec " << P.colrec << "\ncoupling " << P.coupling << "\nnrec_real "
        << P.nrec_real << "\nndrec_real " << P.ndrec_real << "\n";
    if (P.outcome != PlanOutcome::accepted) return 0;
    save("prow.i64", P.prow);
    save("grow.i64", P.grow);
    save("drow.i64", P.drow);
    save("rowptr.i64", P.rowptr);
    save("pcol.i32", P.pcol);
    save("gcol.i32", P.gcol);
    save("dcol.i32", P.dcol);
    save("col.i32", P.col);
    save("pkc.f64", P.pkc);
    save("gxy.f64", P.gxy);
    save("gz.f64", P.gz);
    save("dxy.f64", P.dxy);
    save("dz.f64", P.dz);
    save("val.f64", P.val);
    save("plen.i32", P.plen);
    save("dlen.i32", P.dlen);
    // the ordinary tiles as build_tiles (csr.hip) makes them: boundaries, descriptors, tiles without ghost columns first
    TileInput in;
    in.m = P.m;
    in.order = o;
    in.rowptr = P.rowptr.data();
    in.prow = P.prow.data();
    in.grow = P.colrec ? P.grow.data() : nullptr;
    in.drow = P.coupling ? P.drow.data() : nullptr;
    in.num_cu = (int)meta["num_cu"];
    std::vector<int32_t> tp;
    const PlanOutcome fit = plan_tile_boundaries(in, caps.tile_slots, caps.tile_rows, caps.tile_rows, tp);
    out << "tiles_fit " << (int)fit << "\n";
    if (fit != PlanOutcome::accepted) return 0;
    const std::vector<PlanTile> td = plan_tiles(in, tp);
    std::vector<PlanTile> ord;
    int32_t interior = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (const PlanTile &t : td) {
            const std::vector<int32_t> &cc = (P.colrec && t.r0 < o.block_rows()) ? P.gcol : P.col;
            bool ghost = false;
            for (int64_t k = t.base; k < t.base + t.n; ++k) ghost = ghost || cc[(size_t)k] >= P.m;
            if (ghost == (pass == 1)) ord.push_back(t);
        }
        if (pass == 0) interior = (int32_t)ord.size();
    }
    save_tiles("tiles.i64", ord);
    out << "tiles_interior " << interior << "\n";
    GhostNodes gn{load<int32_t>("gn_col.i32"), load<int32_t>("gn_ncomp.i32")};
    const WindowPlan W = plan_window_tiles(P, gn, in.num_cu, ord, interior, sw, caps);
    out << "win_present " << W.present << "\nwin_overflow " << W.overflow << "\nwin_own " << W.own << "\nwin_rows_own " << W.rows_own
        << "\nwin_ninterior " << W.ninterior << "\nwin_nrow_tiles " << W.nrow_tiles << "\nwin_wlanes " << W.wlanes << "\nwin_npairs "
        << W.npairs << "\nwin_ndpairs " << W.ndpairs << "\nwin_nw_rec " << W.nw_rec << "\nwin_nw_grec " << W.nw_grec << "\nwin_nw_drec "
        << W.nw_drec << "\n";
    if (!W.present) return 0;
    save_tiles("wtiles.i64", W.tiles);
    save("widx.u16", W.widx);
    save("gidx.u16", W.gidx);
    save("dwidx.u16", W.dwidx);
    save("wlist.i32", W.wlist);
    save("vlist.i32", W.vlist);
    save("wbk.i32", W.wbk);
    save("dbk.i32", W.dbk);
    save("pkc2.f64", W.pkc2);
    save("dxy2.f64", W.dxy2);
    save("wgval.f64", W.wgval);
    save("wdz.f64", W.wdz);
    save("gslot.i32", W.gslot);
    save("wprow.i64", W.prow);
    save("wgrow.i64", W.grow);
    save("wdrow.i64", W.drow);
    save("wpcol.i32", W.pcol);
    save("wgcol.i32", W.gcol);
    save("wdcol.i32", W.dcol);
    return 0;
}
