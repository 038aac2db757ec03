// paths_driver.cpp -- prints what outerspace_amd/csrc/osp_paths.h decides for one product, as one JSON line:
//   paths_driver <algorithm> <nnz> <p_all> <M> <N> <partials_only> <split_row_max> <direct_dense_max>
// with the OSP_* settings taken from the environment.  Built by tests/test_paths_cpu.py, plain and under AddressSanitizer +
// UBSan.  Includes nothing else of the library.
#include <cstdio>
#include <cstdlib>

#include "../outerspace_amd/csrc/osp_paths.h"

using namespace osp;

int main(int argc, char **argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: %s algorithm nnz p_all M N partials_only split_row_max direct_dense_max\n", argv[0]);
        return 2;
    }
    uint64_t a[9] = {0};
    for (int i = 1; i < 9; i++) a[i] = strtoull(argv[i], nullptr, 10);
    const ProductPaths p = choose_paths(Settings::read(), (int)a[1], a[2], a[3], a[4], a[5], a[6] != 0, PathLimits{a[7], a[8]});
    const auto b = [](bool v) { return v ? "true" : "false"; };
    printf("{\"rowwise\": %s, \"direct\": %s, \"direct_max\": %llu, \"direct_min_nnz\": %llu, \"gather_long\": %s, \"gather_short\": %s, "
           "\"av_ride_along\": %s, \"keep_table\": %s, \"expand_rows\": %s}\n",
           b(p.rowwise), b(p.direct), (unsigned long long)p.direct_max, (unsigned long long)p.direct_min_nnz, b(p.gather_long),
           b(p.gather_short), b(p.av_ride_along), b(p.keep_table), b(p.expand_rows));
    return 0;
}
