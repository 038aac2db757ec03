/*
 * outerspace_spgemm_vector.h -- where a CSR result meets a dense per-vertex vector, on an AMD Instinct MI355X (gfx950):
 * reduce a result's rows or columns to a vector, combine a result's values with a vector per row and a vector per column,
 * and keep the entries whose row and column pass a per-vertex verdict.
 *
 * The other CSR-to-CSR operations (inflate_prune, apply_mask, select, ewise) take matrices and return a matrix.  These are
 * the three remaining primitives between them and degrees, k-core, Jaccard similarity and the clustering coefficient
 * (outerspace_amd/graph.py).  It adds THREE functions and changes no existing struct (OSP_VERSION stays as
 * outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 *
 * For all three: `in` is any CSR result that is not one of osp_spgemm_partials, and it stays valid.  Everything runs on the
 * context's stream with temporary buffers from its pool.  Vectors hold values of `in`'s dtype (keep vectors: bytes) and lie
 * in `space`.  OSP_ERR_ARG: a null `in`, a null required output pointer, a value outside its enum, a bad space, a non-zero
 * reserved word, a result of osp_spgemm_partials, and -- for the column axis and the vertex select -- an `in` of 2^32 - 1
 * entries or more (positions are kept in 32 bits, as osp_csr_apply_mask keeps its mask's).  On any error *out, the output
 * vector and *stats are left as they were.  An empty `in` and M == 0 are legal and launch no kernel.
 */
#ifndef OUTERSPACE_SPGEMM_VECTOR_H
#define OUTERSPACE_SPGEMM_VECTOR_H

#include "outerspace_spgemm.h"
#include "outerspace_spgemm_ewise.h"   /* osp_ewise_op_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSP_AXIS_ROWS = 0,   /* one value per row: M values */
    OSP_AXIS_COLS = 1    /* one value per column: N values */
} osp_axis_t;

typedef enum {
    OSP_REDUCE_PLUS = 0,
    OSP_REDUCE_MIN = 1,
    OSP_REDUCE_MAX = 2,
    OSP_REDUCE_COUNT = 3
} osp_reduce_op_t;

#define OSP_VECTOR_NONE (-1)

typedef struct osp_vector_apply {
    int32_t  row_op;        /* osp_ewise_op_t or OSP_VECTOR_NONE */
    int32_t  col_op;        /* osp_ewise_op_t or OSP_VECTOR_NONE */
    uint32_t reserved[8];   /* must be 0 */
} osp_vector_apply_t;

typedef struct osp_vector_stats {
    uint64_t nnz_in;          /* entries of `in` */
    uint64_t nnz_out;         /* entries of `out` (reduce: values of the output vector) */
    uint64_t long_segments;   /* reduce: rows / columns longer than one block of 2048 entries */
    float    ms_total;        /* device time of the call */
    uint32_t launches;        /* kernels launched (copies not counted) */
    uint32_t reserved[6];     /* written 0 */
} osp_vector_stats_t;

/*
 * out_vec[i] = the reduction of row i (OSP_AXIS_ROWS, M values) or of column i (OSP_AXIS_COLS, N values) of `in`, in `in`'s
 * dtype, in `space`.  The result is DEFINED TO THE BIT, as osp_csr_inflate_prune defines its sums.
 *
 * A SEGMENT is a row's entries in ascending column order, or a column's entries in ascending row order.  `id` is +0.0 for
 * PLUS, +inf for MIN, -inf for MAX.  a (+) b is a + b (one IEEE addition, never contracted) for PLUS, b < a ? b : a for MIN,
 * b > a ? b : a for MAX.  R(e_0 .. e_{m-1}) is formed as follows.
 *   m <= 2048:  for every lane l in 0..63, p_l = id; then p_l = p_l (+) e_{l + 64 t} for t = 0, 1, .. while the element
 *               exists; then for d in 32, 16, 8, 4, 2, 1: p_l = p_l (+) p_{l + d} for l < d.  The result is p_0.
 *               (This is the order in which osp_csr_inflate_prune sums a row.)
 *   m > 2048:   the sequence is cut into consecutive blocks of 2048, the last one shorter; r_b = R(block b); the result is
 *               R(r_0 .. r_{ceil(m / 2048) - 1}), recursively.
 * Consequences: an empty segment gives `id`; MIN and MAX never return a NaN and always return one entry's bits or `id` (a
 * comparison with a NaN is false, so a NaN entry is never taken); PLUS propagates NaN, and a lone -0.0 sums to +0.0
 * (+0.0 + -0.0); the order depends on the segment's length alone, not on where it lies in the arrays or on the other
 * segments; COUNT is the segment's length converted to the dtype, (T)m, and reads no value.
 *
 * The column axis first takes the column-major view of `in` by one stable sort by column (entries of one column keep
 * ascending row order), then reduces that view's segments as rows are reduced.
 *
 * stats (may be NULL): nnz_in, nnz_out = M or N, long_segments = segments of more than 2048 entries, ms_total, launches,
 * reserved = 0.
 */
int osp_csr_reduce(osp_result_t in, int axis /* osp_axis_t */, int op /* osp_reduce_op_t */, void *out_vec, osp_memspace_t space,
                   osp_vector_stats_t *stats /* may be NULL */);

/*
 * out has in's pattern (rowptr and colidx are copied), and the value at (i, j) is col_op(row_op(c, x_rows[i]), y_cols[j])
 * with c = in's value there.
 *
 * Each op is the ONE IEEE operation of osp_csr_ewise's table, with c (or the intermediate) in a's place and the vector's
 * element in b's: PLUS c + x, TIMES c * x, MINUS c - x, DIV c / x, MIN x < c ? x : c, MAX x > c ? x : c (a copy of one
 * operand's bits; with a NaN in either place c is kept), SECOND x's bits.  An op of OSP_VECTOR_NONE skips that side, and its
 * vector pointer is then ignored.  SECOND never loads `in`'s value when it is the first side applied.
 *   x_rows -- M values, y_cols -- N values of in's dtype, in `space`
 *
 * OSP_ERR_ARG beyond the common cases: a null ap; OSP_EWISE_FIRST (it would be a copy); both sides NONE; a side with an op
 * and a null vector.
 *
 * stats (may be NULL): nnz_in = nnz_out, long_segments = 0, ms_total, launches, reserved = 0.
 */
int osp_csr_apply_vectors(osp_result_t in, const osp_vector_apply_t *ap, const void *x_rows, const void *y_cols, osp_memspace_t space,
                          osp_result_t *out, osp_vector_stats_t *stats /* may be NULL */);

/*
 * out = the entries (i, j) of `in` with (keep_rows == NULL or keep_rows[i] != 0) and (keep_cols == NULL or
 * keep_cols[j] != 0): the subgraph induced by a vertex set when both vectors are that set's indicator.
 *   keep_rows -- M bytes, keep_cols -- N bytes, in `space`; either may be NULL, both NULL is OSP_ERR_ARG
 *
 * The shape does not change: a removed vertex is an empty row or an empty column, nothing is renumbered.  Kept values are
 * copied bit for bit.  Row pointers are exact and out is allocated at its exact size, the contract of osp_csr_select.
 *
 * stats (may be NULL): nnz_in, nnz_out, long_segments = 0, ms_total, launches, reserved = 0.
 */
int osp_csr_select_vertices(osp_result_t in, const uint8_t *keep_rows, const uint8_t *keep_cols, osp_memspace_t space,
                            osp_result_t *out, osp_vector_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_VECTOR_H */
