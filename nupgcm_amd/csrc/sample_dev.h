// The locator's and the located points' handles, shared by the translation units that locate and evaluate points (sample.hip: point
// sampling and grid integrals; particles.hip: particle advection; surfaces.hip).  sample_point reads the engine's tables through the
// cell view (DevCells, fe_dev.h).
#pragma once
#include "common.h"
#include "fe_dev.h"
#include "sample_core.h"

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
