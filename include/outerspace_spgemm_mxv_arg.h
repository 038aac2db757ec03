/*
 * outerspace_spgemm_mxv_arg.h -- osp_csr_mxv under MIN or MAX together with WHERE the winning product is, on an AMD
 * Instinct MI355X (gfx950): y = in (add.mul) x and arg[i] = the column of row i's smallest (largest) product, in one fused
 * pass over `in`, without leaving the device.
 *
 * The lightest edge leaving a vertex (Boruvka), the heaviest free neighbour (handshake matching), the nearest neighbour: the
 * positional operators of GraphBLAS (secondi / firstj) under a MIN or MAX monoid.  Composed from what was there it takes two
 * osp_csr_mxv calls and an osp_csr_apply_vectors / osp_csr_select round trip, which writes a copy of the matrix per step.
 * This header includes outerspace_spgemm_mxv.h, adds ONE function and changes no existing struct (OSP_VERSION stays as
 * outerspace_spgemm.h gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MXV_ARG_H
#define OUTERSPACE_SPGEMM_MXV_ARG_H

#include "outerspace_spgemm_mxv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_mxv_arg_stats {
    uint64_t nnz_in;         /* entries of `in` */
    uint64_t nnz_out;        /* M */
    uint64_t long_segments;  /* rows of more than 2048 entries */
    uint64_t rows_without;   /* rows whose arg is -1: empty, or every product a NaN */
    uint32_t group;          /* lanes per row of the packed path this call used: 4, 8, 16, 32, or 64 (no packing) */
    uint32_t launches;       /* kernels launched, copies not counted */
    float    ms_total;       /* device time of the call */
    uint32_t reserved[7];    /* written 0 */
} osp_mxv_arg_stats_t;

/*
 * With p_t = mul(in[i, j_t], x[j_t]) over the entries of row i in ascending column order -- exactly osp_csr_mxv's
 * products: ONE IEEE operation of osp_csr_ewise's table, nothing contracted --
 *   y[i]   = R_add(p_0 .. p_{m-1}), osp_csr_mxv's y for the same arguments BIT FOR BIT (the sign of a zero and the identity
 *            of a row with nothing to take included);
 *   arg[i] = the smallest column j_t among the products that are not NaN and for which no other non-NaN product is
 *            smaller (add = MIN) or larger (add = MAX) under the IEEE comparison; -1 when the row is empty or every product
 *            is a NaN.
 *
 *   in    -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   sr    -- add is MIN or MAX (PLUS and FIRST are refused: a sum has no position); mul is TIMES, PLUS, MIN, MAX, FIRST or
 *            SECOND (osp_csr_mxv's six); the reserved words must be 0
 *   x     -- N values of in's dtype in `space`; may be NULL when mul is FIRST: the call is then the arg-reduce of the rows
 *            of `in` itself.  mul = SECOND loads no value of `in`, mul = FIRST loads no x.
 *   y     -- M values of in's dtype in `space`, or NULL: the caller wants positions only
 *   arg   -- M int64 values in `space`
 *
 * Ties and special values.  -0.0 and +0.0 are EQUAL under the IEEE comparison: a tie between them goes to the smaller
 * column, whichever sign y carries (y's sign is osp_csr_mxv's).  A NaN product never wins and never ties.  A row whose only
 * non-NaN product equals the identity (+inf under MIN, -inf under MAX) reports that product's column, not -1: -1 says
 * "nothing to take", which y alone cannot say.
 *
 * arg does NOT depend on the order of the reduction.  (value, column) under "better value, then smaller column" is a total
 * preorder (values compare as numbers, so the two zeros are one value), and arg is the column of its minimum; a minimum is
 * associative and commutative.  So neither the reduction tree, nor the group g, nor where a long row is cut into blocks
 * changes any arg -- and none of them changes a bit of y, as outerspace_spgemm_mxv.h states.
 *
 * y and arg are formed in pool buffers and copied out last: x == y is legal when M == N, and a call that fails leaves y,
 * arg and *stats as they were.  OSP_ERR_ARG: a null in, sr or arg; a null x unless mul is FIRST; an operator outside its
 * list; a non-zero reserved word; a bad space; a result of osp_spgemm_partials.  M == 0 or an `in` without entries launches
 * nothing: arg is then M times -1 and y M identities.  The column axis is osp_csr_transpose first: there is no axis
 * argument.
 *
 * Rows of at most g entries are packed 64 / g to a wave, g chosen as osp_csr_mxv chooses it and forced by the same
 * OSP_MXV_GROUP (environment, read per call: INTEGRATION.md section 7); rows of more than 2048 entries go through blocks
 * of 2048 and a second level on (value, column) pairs, recursively.  Everything runs on the context's stream with temporary
 * buffers from its pool; no float atomics, no waiting between workgroups; the read-backs are rows_without and, only when
 * `in` has more than 2048 entries, the number of long rows per level.
 *
 * stats (may be NULL): as commented in the struct.
 */
int osp_csr_mxv_arg(osp_result_t in, const osp_semiring_t *sr, const void *x, void *y /* may be NULL */, int64_t *arg,
                    osp_memspace_t space, osp_mxv_arg_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MXV_ARG_H */
