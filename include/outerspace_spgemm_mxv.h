/*
 * outerspace_spgemm_mxv.h -- a CSR result times a dense vector under a named semiring on an AMD Instinct MI355X (gfx950):
 * y = in (add.mul) x, one fused pass over `in`, without leaving the device.
 *
 * The step of every power iteration (PageRank, label propagation, Bellman-Ford with a dense distance vector).  It can be
 * composed from osp_csr_apply_vectors and osp_csr_reduce, which writes a copy of the matrix per step; this function reads
 * `in` once and writes M values.  The semiring is osp_semiring_t of outerspace_spgemm_mxm.h, which this header includes.  It
 * adds ONE function and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h gives it).  No reference
 * counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MXV_H
#define OUTERSPACE_SPGEMM_MXV_H

#include "outerspace_spgemm_mxm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_mxv_stats {
    uint64_t nnz_in;         /* entries of `in` */
    uint64_t nnz_out;        /* M */
    uint64_t long_segments;  /* rows of more than 2048 entries */
    uint32_t group;          /* lanes per row of the packed path this call used: 4, 8, 16, 32, or 64 (no packing) */
    uint32_t launches;       /* kernels launched, copies not counted */
    float    ms_total;       /* device time of the call */
    uint32_t reserved[7];    /* written 0 */
} osp_mxv_stats_t;

/*
 * y[i] = R_add(p_0 .. p_{m-1}), p_t = mul(in[i, j_t], x[j_t]) over the entries of row i in ascending column order.
 *   in    -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   sr    -- add is PLUS, MIN or MAX (the value operators of osp_csr_reduce; FIRST is refused); mul is TIMES, PLUS, MIN, MAX,
 *            FIRST or SECOND (MINUS and DIV are refused, as in osp_csr_mxm); the reserved words must be 0
 *   x     -- N values of in's dtype in `space`; may be NULL when mul is FIRST
 *   y     -- M values of in's dtype in `space`
 *
 * The result is DEFINED TO THE BIT.  R is the reduction of outerspace_spgemm_vector.h (64 lane values, the butterfly
 * 32 .. 1, blocks of 2048, recursive) with its identities: an empty row gives +0.0 for PLUS, +inf for MIN, -inf for MAX.  mul
 * is the ONE IEEE operation of osp_csr_ewise's table with the entry in a's place and x[j] in b's.  A product and the addition
 * after it are two roundings: nothing is contracted.  MIN and MAX never return a NaN; PLUS propagates it.  mul = SECOND
 * never loads in's values, mul = FIRST never loads x (nor in's columns).
 *
 * For every legal semiring y equals, bit for bit, osp_csr_reduce(OSP_AXIS_ROWS, add) of
 * osp_csr_apply_vectors(col_op = mul, y_cols = x) of `in`; for mul = FIRST it equals osp_csr_reduce(OSP_AXIS_ROWS, add) of
 * `in` itself.  (R's order depends on a row's length alone, so how the rows are cut over the device changes no bit.)
 *
 * y is formed in a pool buffer and copied out last: x == y is legal when M == N (an iteration may overwrite its vector), and
 * a call that fails leaves y and *stats as they were.  OSP_ERR_ARG: a null in, sr or y; a null x unless mul is FIRST; an
 * operator outside its list; a non-zero reserved word; a bad space; a result of osp_spgemm_partials.  M == 0 or an `in`
 * without entries launches nothing: y is then M identities.
 *
 * Rows of at most g entries are packed 64 / g to a wave, g in {4, 8, 16, 32, 64} chosen per call from nnz / M (no
 * read-back); OSP_MXV_GROUP (environment, read per call: INTEGRATION.md section 7) forces g.  g changes no bit of y.  Everything runs on the context's
 * stream with temporary buffers from its pool; no float atomics, no waiting between workgroups; the only read-back is the
 * number of rows of more than 2048 entries per level, and only when `in` has more than 2048 entries.
 *
 * stats (may be NULL): as commented in the struct.
 */
int osp_csr_mxv(osp_result_t in, const osp_semiring_t *sr, const void *x, void *y, osp_memspace_t space,
                osp_mxv_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MXV_H */
