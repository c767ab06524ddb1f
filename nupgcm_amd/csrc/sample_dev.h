// The locator's and the located points' handles and the engine's tables as sample_point reads them, shared by the translation units
// that locate and evaluate points (sample.hip: point sampling and grid integrals; particles.hip: particle advection).
#pragma once
#include "common.h"
#include "fe_dev.h"
#include "sample_core.h"

namespace npg {

// the engine's tables as sample_point reads them ([component][cell])
struct DevTables {
    const int32_t *cu_, *cp_, *cb_;
    const double *G_, *udiri, *bdiri;
    int64_t ncell;
    int nb;
    __device__ __forceinline__ int32_t cu(int l, int64_t c) const { return cu_[(size_t)l * ncell + c]; }
    __device__ __forceinline__ int32_t cp(int m, int64_t c) const { return cp_[(size_t)m * ncell + c]; }
    __device__ __forceinline__ int32_t cb(int i, int64_t c) const { return cb_[(size_t)i * ncell + c]; }
    __device__ __forceinline__ double G(int k, int64_t c) const { return G_[(size_t)k * ncell + c]; }
};

}  // namespace npg

struct npg_locator {
    npg_ctx *ctx = nullptr;
    int64_t ncell = 0;           // cells of the engine it serves; partitioned: 1 + the largest engine index among its records
    bool part = false;           // npg_locator_create_cells: records = owned cells + witness layer (sample_core.h, locate_point<true>)
    int64_t nrec = 0, nowned = 0;
    npg::BinGrid grid{};
    int32_t *bin_ptr = nullptr, *bin_cells = nullptr;
    double *geo = nullptr;
    int64_t nentries = 0, max_per_bin = 0;
    double *grid_part = nullptr;     // npg_fe_grid_integrals: the zonal partials [nchunk][kGridZon][ny][nz], grown on demand
    size_t grid_part_n = 0;
};

struct npg_located {
    npg_ctx *ctx = nullptr;
    int64_t n = 0;
    int32_t *cell = nullptr;     // [n]
    double *lam = nullptr;       // [n][4]
};
