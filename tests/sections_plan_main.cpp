// Stand-alone driver of the section planner (nupgcm_amd/csrc/sections_core.h) for tests/test_sections_plan.py: reads one case as raw
// little-endian arrays from a directory, plans, writes every array of the plan back.  No GPU, no HIP: built with g++ under
// AddressSanitizer and UBSan by the test.
//   sections_plan_main DIR        DIR/meta.txt: "key value" lines (ncell, nsec); DIR/{cell_xyz.f64, frames.f64, n1.i32, n2.i32,
//                                 edges1.f64, edges2.f64[, mask.u8]}
// Writes DIR/out_meta.txt (status 0 and the counters, or status 1), DIR/out_message.txt and DIR/out_{cell.i32, bin.i32, sec.u8, lam.f64,
// area.f64, bin_ptr.i64, sec_bin0.i64}.
#include <cstdio>
#include <fstream>
#include <map>
#include <string>

#include "../include/nupgcm_hip.h"                       // (the field codes that the headers behind mixing_core.h read)
#include "../nupgcm_amd/csrc/sections_core.h"

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
    const std::vector<double> xyz = load<double>("cell_xyz.f64"), frames = load<double>("frames.f64");
    const std::vector<double> e1 = load<double>("edges1.f64"), e2 = load<double>("edges2.f64");
    const std::vector<int32_t> n1 = load<int32_t>("n1.i32"), n2 = load<int32_t>("n2.i32");
    const std::vector<uint8_t> mask = load<uint8_t>("mask.u8");
    SecPlan pl;
    const std::string msg = sec_build_plan(true, false, (int64_t)meta["ncell"], xyz.data(), (int)meta["nsec"], frames.data(), n1.data(), n2.data(),
                                           e1.data(), e2.data(), mask.empty() ? nullptr : mask.data(), pl);
    std::ofstream out(dir + "/out_meta.txt");
    std::ofstream(dir + "/out_message.txt") << msg << "\n";
    if (!msg.empty()) {
        out << "status 1\n";
        return 0;
    }
    out << "status 0\nnpiece " << pl.npiece() << "\nnbin " << pl.nbin << "\nncut_cells " << pl.ncut_cells << "\nmax_per_bin " << pl.max_per_bin << "\n";
    save("cell.i32", pl.cell);
    save("bin.i32", pl.bin);
    save("sec.u8", pl.sec);
    save("lam.f64", pl.lam);
    save("area.f64", pl.area);
    save("bin_ptr.i64", pl.bin_ptr);
    save("sec_bin0.i64", pl.sec_bin0);
    return 0;
}
