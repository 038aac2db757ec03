// osp_paths.h -- which formulation a product runs: ONE struct of decisions and one function that derives them (DESIGN.md
// section 28).  Host only, no HIP: osp_api.hip and tests/paths_driver.cpp include it as plain C++.
//
// The four formulations: outer products staged and split afterwards; the row-wise variant; direct rows (long rows written
// straight into their column ranges by the multiply); gathered rows (the merge kernel forms the products itself, from run
// descriptors) -- long rows only, or short rows too.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/outerspace_spgemm.h"
#include "osp_settings.h"

namespace osp {

// the device constants the choice reads (osp_split.h: kSplitRowMax, kDirectDenseMax)
struct PathLimits {
    uint64_t split_row_max;     // longest row one workgroup splits: the default of OSP_DIRECT_MAX
    uint64_t direct_dense_max;  // the planner counts a row's products in 21 bits: the cap of OSP_DIRECT_MAX
};

struct ProductPaths {
    // Row-wise variant (cfg.algorithm): rows of up to one tile of partial products are computed inside the tile kernel
    // from the chunk table
    bool rowwise = false;
    // Long rows that one workgroup could split are written straight into their column ranges by the multiply phase
    // ("direct" rows, osp_split.h).  OSP_DIRECT=0 switches that off (every long row is then split after the multiply, as
    // the parts-merging entry points do), OSP_DIRECT_MAX=<partial products> bounds the rows it applies to.
    bool direct = false;
    uint64_t direct_max = 0, direct_min_nnz = 0;
    // Gathered rows (osp_kernels.h): the merge kernel forms the partial products of planned long rows and of short rows
    // itself, from run descriptors; on unless OSP_GATHER=0 (debugging aid, A/B timing: every row is then written by the
    // multiply, as until round 4) or the row-wise variant runs (its tile kernel is another instantiation).  OSP_GATHER=1:
    // long rows only.
    bool gather_long = false, gather_short = false;
    // (gathered rows: the A values ride along in the symbolic sort, so that the run descriptors' makers read them in
    // (row, k) order -- wherever long rows are gathered)
    bool av_ride_along = false;
    bool keep_table = false;    // the chunk table -- (length, B row) pairs in (row, k) order -- outlives the symbolic phase
    // the short rows are gathered too: plainly staged long rows are expanded row by row, and the chunk offsets are made
    // lazily, where only rows written through cells would read them (DirectSrc::ensure_chunk_off)
    bool expand_rows = false;
};

// nnz: the non-zeros of A inside the shard; p_all: the partial products of the whole product.
inline ProductPaths choose_paths(const Settings &env, int algorithm, uint64_t nnz, uint64_t p_all, uint64_t M, uint64_t N,
                                 bool partials_only, const PathLimits &lim) {
    ProductPaths p;
    // Small products keep the split: the plan costs a handful of launches and a read-back, which a product of a few
    // milliseconds does not earn back (web-Google shape: 2.3 ms with the split, 2.7 with direct rows).  OSP_DIRECT_MIN_NNZ
    // moves that boundary (the tests set it to 0, so that their small inputs take the direct path).
    p.direct_min_nnz = env.direct_min_nnz.or_((env.gather.set && env.gather.value == 0) ? (8ull << 20) : (2ull << 20));
    p.direct_max = std::min<uint64_t>(env.direct_max.or_(lim.split_row_max), lim.direct_dense_max);
    if (nnz == 0 || partials_only) return p;   // nothing to choose: no chunk, or the multiply phase alone
    p.rowwise = algorithm == OSP_ALGO_ROWWISE;
    // ... unless its output rows are dense on average (at least 0.375 partial products per entry of the M x N result -- three
    // times the density from which a long row's column ranges are capped at the dense accumulators' width, plan_panel):
    // such rows are written in a few wide ranges, long runs, and summed without a sort -- 4096^2 with 880 entries per row
    // (3.6 M non-zeros, 3.2 G partial products) 44.4 -> 26.4 ms, Graph500 scale 14 ef 512 100 -> 79 ms.
    const bool dense_avg = (long double)p_all * 8.0L >= 3.0L * (long double)M * (long double)N;
    p.direct = (nnz >= p.direct_min_nnz || dense_avg) && env.direct.on;
    const int gather_env = env.gather.or_(2);
    p.gather_long = !p.rowwise && gather_env >= 1 && p.direct;
    // (short rows: only where long rows are planned too -- a product of a few million non-zeros does not earn the tables
    // back: web-Google shape 2.09 -> 2.50 ms with them)
    p.gather_short = !p.rowwise && gather_env >= 2 && p.direct;
    p.av_ride_along = p.gather_long;
    p.keep_table = p.rowwise || p.direct;
    p.expand_rows = p.gather_short && env.expand_rows.on;
    return p;
}

}  // namespace osp
