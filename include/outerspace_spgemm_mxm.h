/*
 * outerspace_spgemm_mxm.h -- the product of two CSR results under a named semiring on an AMD Instinct MI355X (gfx950):
 * out = a (add.mul) b, row by row (Gustavson), without leaving the device.
 *
 * Every other product of this library adds with + and multiplies with x, and takes its operands through the ingest of the
 * outer-product pipeline.  This one takes two results as they lie in HBM -- both CSR, columns ascending -- so nothing is
 * ingested, transposed or viewed, and the two operators are chosen from the table of outerspace_spgemm_ewise.h, which this
 * header includes.  A sparse frontier times a graph under (MIN, PLUS) is the shape it is for.  It adds ONE function and
 * changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MXM_H
#define OUTERSPACE_SPGEMM_MXM_H

#include "outerspace_spgemm_ewise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_semiring {
    int32_t  add;           /* osp_ewise_op_t: PLUS, MIN, MAX or FIRST */
    int32_t  mul;           /* osp_ewise_op_t: TIMES, PLUS, MIN, MAX, FIRST or SECOND */
    uint32_t reserved[8];   /* must be 0 */
} osp_semiring_t;

typedef struct osp_mxm_stats {
    uint64_t nnz_a, nnz_b;  /* entries of the operands */
    uint64_t products;      /* sum over entries A[i,k] of nnz(B[k,:]) */
    uint64_t nnz_out;       /* entries of `out` */
    uint64_t short_rows, long_rows;   /* output rows by class (below); rows without a product are in neither */
    uint32_t batches;       /* row batches the call was cut into */
    uint32_t launches;      /* kernels launched (copies not counted) */
    float    ms_total;      /* device time of the call */
    uint32_t reserved[7];   /* written 0 */
} osp_mxm_stats_t;

/*
 * out = a (add.mul) b.
 *   a, b -- CSR results (not results of osp_spgemm_partials) of the same context and dtype, a M x K and b K x N; both stay
 *           valid; a == b (the same handle) is legal
 *   sr   -- the two operators
 *
 * Row i of out has an entry at column j if and only if at least one k has a stored A[i,k] and a stored B[k,j].  This is
 * structural: an explicit zero is an entry like any other, and a value that cancels stays an entry.  Its value is formed
 * from the products p_t = mul(A[i,k_t], B[k_t,j]), k_0 < k_1 < ... the common k in ascending order:
 *     acc = p_0;  acc = add(acc, p_t) for t = 1, 2, ...   (left to right)
 * mul and add are each ONE IEEE operation of the table in outerspace_spgemm_ewise.h in the results' dtype, with A's value
 * (or acc) in a's place and B's value (or p_t) in b's: PLUS a + b, TIMES a * b, MIN b < a ? b : a, MAX b > a ? b : a,
 * FIRST a's bits, SECOND b's bits.  Nothing is contracted: a product and the addition after it are two roundings.  The
 * fold starts AS the first product, not from an identity: a lone -0.0 stays -0.0, MIN over NaNs keeps p_0, and
 * add = FIRST is "the product of the smallest k" (a deterministic ANY).
 *
 * With (PLUS, TIMES) out equals the result of osp_spgemm_coo / osp_spgemm_csc_csr of the same operands in row pointers,
 * columns and value bits: that product also sums left to right in ascending k from the first product.
 *
 * Columns ascend in every row, row pointers are exact, and out is allocated at its exact size.  out is an ordinary
 * osp_result_t on the operands' context, taken by every osp_result_* and osp_csr_* function, this one included.
 * osp_result_info(out): M, K, N of the call, row_begin = 0, row_end = M, nnz_a, nnz_b, nnz_c, partials = the number of
 * products, dtype and ms_total; every other field is 0.
 *
 * Rows are processed in consecutive batches of at most OSP_MXM_BATCH products (environment, read per call: INTEGRATION.md section 7; default 2^24);
 * a single row with more is a batch of its own.  Temporary memory follows the batch, not the product count.  An output row
 * of at most OSP_MXM_SHORT_CAP products (default 1024, at most 1024) is SHORT: one wave forms, sorts and folds it in LDS.
 * A row with more is LONG: its products are expanded to a pool buffer, sorted by (row, column) with the library's stable
 * radix sort and folded run by run, the work cut by products over the whole device.
 *
 * OSP_ERR_ARG: a null a, b, sr or out; an add or mul outside its list above (MINUS and DIV included); a non-zero reserved
 * word; operands of different contexts or dtypes; a result of osp_spgemm_partials; an operand of 2^32 - 1 entries or more.
 * OSP_ERR_DIM: a's N differs from b's M.  OSP_ERR_CAPACITY: ONE output row with 2^32 - 1 products or more (positions
 * inside a batch are 32 bits; the total over all rows is not limited by this).  On any error *out and *stats are left as
 * they were.  M == 0, an empty a, an empty b and a product count of 0 (every k of a meets an empty row of b) are legal,
 * launch no numeric kernel and give an empty M x N result.
 *
 * stats (may be NULL): as commented in the struct.
 */
int osp_csr_mxm(osp_result_t a, osp_result_t b, const osp_semiring_t *sr, osp_result_t *out, osp_mxm_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MXM_H */
