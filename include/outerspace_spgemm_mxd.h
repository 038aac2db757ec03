/*
 * outerspace_spgemm_mxd.h -- a CSR result times a dense matrix under a named semiring on an AMD Instinct MI355X (gfx950):
 * Y = in (add.mul) X with X dense N x k and Y dense M x k, both row-major and contiguous, one pass over `in`, without
 * leaving the device.
 *
 * The step of feature propagation (A^ X), label spreading, block power iterations and every "k sources at once" iteration
 * whose iterate has filled in.  It can be composed from k calls of osp_csr_mxv on contiguous columns, which reads `in` k
 * times; this function reads it once per 64 columns.  The semiring is osp_semiring_t of outerspace_spgemm_mxm.h, which this
 * header includes.  It adds ONE function and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h gives it).
 * No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MXD_H
#define OUTERSPACE_SPGEMM_MXD_H

#include "outerspace_spgemm_mxm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSP_MXD_MAX_COLS 65536u /* the largest k */

typedef struct osp_mxd_stats {
    uint64_t nnz_in;         /* entries of `in` */
    uint64_t nnz_out;        /* M * k */
    uint64_t cols;           /* k */
    uint64_t long_segments;  /* rows of more than 2048 entries */
    uint32_t lanes_per_row;  /* lanes a row gets in a wave: the power of two >= min(k, 64); 64 / lanes_per_row rows per wave */
    uint32_t launches;       /* kernels launched, copies not counted */
    float    ms_total;       /* device time of the call */
    uint32_t reserved[7];    /* written 0 */
} osp_mxd_stats_t;

/*
 * y[i, c] = R_add(p_0 .. p_{m-1}), p_t = mul(in[i, j_t], x[j_t, c]) over the entries of row i in ascending column order.
 *   in    -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   sr    -- osp_csr_mxv's operators: add is PLUS, MIN or MAX; mul is TIMES, PLUS, MIN, MAX, FIRST or SECOND; the reserved
 *            words must be 0
 *   x     -- N x k values of in's dtype in `space`, row-major, contiguous (x[j, c] at j * k + c); may be NULL when mul is
 *            FIRST
 *   k     -- the number of columns, at most OSP_MXD_MAX_COLS
 *   y     -- M x k values of in's dtype in `space`, row-major, contiguous
 *
 * The result is DEFINED TO THE BIT: column c of y equals osp_csr_mxv(in, sr, column c of x) bit for bit, for every legal
 * semiring.  R, its identities (an empty row gives +0.0 for PLUS, +inf for MIN, -inf for MAX) and mul are that function's; a
 * product and the addition after it are two roundings: nothing is contracted.  (R's order depends on a row's length alone;
 * here ONE lane evaluates R's tree for a (row, column) pair, in the tree's own operand order.)
 *
 * y is formed in a pool buffer and copied out last: x == y is legal when M == N (an iteration may overwrite its iterate),
 * and a call that fails leaves y and *stats as they were.  OSP_ERR_ARG: a null in, sr or y; a null x unless mul is FIRST; an
 * operator outside its list; a non-zero reserved word; a bad space; a result of osp_spgemm_partials; k > OSP_MXD_MAX_COLS.
 * k == 0, M == 0 and an `in` without entries are legal and launch nothing: in the last case y is M * k identities.
 *
 * Everything runs on the context's stream with temporary buffers from its pool; no float atomics, no waiting between
 * workgroups; the only read-back is the number of rows of more than 2048 entries, and only when `in` has more than 2048
 * entries.
 *
 * stats (may be NULL): as commented in the struct.  launches is 1 when `in` has at most 2048 entries, else 3 (the zeroing of
 * the counters and the listing of the long rows as well); with a long row it also counts the setup, the scan's kernels, the
 * blocks kernel and the upper kernel.
 */
int osp_csr_mxd(osp_result_t in, const osp_semiring_t *sr, const void *x, uint64_t k, void *y, osp_memspace_t space,
                osp_mxd_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MXD_H */
