/*
 * outerspace_spgemm_mxm_masked.h -- the product of two CSR results under a named semiring AT a mask, on an AMD Instinct
 * MI355X (gfx950): out<mask> = a (add.mul) b or out<NOT mask> = a (add.mul) b, row by row (Gustavson), without leaving the
 * device.
 *
 * osp_csr_mxm (outerspace_spgemm_mxm.h, which this header includes) forms, sorts, folds and writes the whole product, and
 * osp_csr_apply_mask (outerspace_spgemm_apply_mask.h) then throws away what a traversal has no use for.  This call drops a
 * product whose (row, column) the mask rejects WHERE IT IS FORMED: it reaches neither the sort, nor the fold, nor HBM, and
 * its values are never loaded.  A frontier times a graph at the complement of the visited set is the shape it is for.  It
 * adds ONE function and ONE struct and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h gives it).  No
 * reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MXM_MASKED_H
#define OUTERSPACE_SPGEMM_MXM_MASKED_H

#include "outerspace_spgemm_mxm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_mxm_masked_stats {
    uint64_t nnz_a, nnz_b, nnz_mask;  /* entries of the operands and of the mask */
    uint64_t products;        /* as osp_csr_mxm: sum over entries A[i,k] of nnz(B[k,:]) -- a property of a and b alone */
    uint64_t products_kept;   /* the products whose (row, column) the mask admits: what was sorted and folded */
    uint64_t nnz_out;         /* entries of `out` */
    uint64_t short_rows, long_rows;   /* classes by `products` of the row, exactly as osp_csr_mxm reports them */
    uint32_t batches;         /* row batches the call was cut into */
    uint32_t launches;        /* kernels launched (copies not counted) */
    float    ms_total;        /* device time of the call */
    uint32_t reserved[7];     /* written 0 */
} osp_mxm_masked_stats_t;

/*
 * out = the entries of a (add.mul) b at the coordinates the mask admits.
 *   a, b       -- as osp_csr_mxm's: CSR results (not results of osp_spgemm_partials) of the same context and dtype, a M x K
 *                 and b K x N, the same operators
 *   mask       -- an M x N CSR result of the same context.  Only its PATTERN is read: its values and its dtype are
 *                 irrelevant, and an explicit zero in the mask is an entry
 *   complement -- 0: a coordinate is admitted when the mask holds it; non-zero: when the mask does NOT hold it
 *   sr         -- the two operators, as osp_csr_mxm takes them
 * mask == a, mask == b and a == b (the same handles) are all legal, and all three operands stay valid.
 *
 * CONTRACT: out equals  osp_csr_apply_mask(osp_csr_mxm(a, b, sr), mask, complement)  in row pointers, columns and value
 * bits, for every semiring, both dtypes and both senses.  It holds EXACTLY, not within a tolerance, because the mask decides
 * whole output entries -- every product of entry (i, j) has the coordinate (i, j) and so the same verdict -- and the fold of
 * an entry only sees that entry's products, in the same ascending k, starting AS the first of them.  It is structural on
 * both sides: an entry that cancels to zero is kept, and NaN, -0.0 and payloads behave as in osp_csr_mxm.
 *
 * Columns ascend in every row, row pointers are exact, and out is allocated at its exact size.  out is an ordinary
 * osp_result_t on the operands' context, taken by every osp_result_* and osp_csr_* function, this one included.
 * osp_result_info(out) is as osp_csr_mxm's: M, K, N of the call, row_begin = 0, row_end = M, nnz_a, nnz_b, nnz_c,
 * partials = `products` (the FORMED count, not the kept count), dtype and ms_total; every other field is 0.
 *
 * The batches and the row classes (OSP_MXM_BATCH, OSP_MXM_SHORT_CAP, read per call) are defined by FORMED products exactly as
 * in osp_csr_mxm, so stats' products, short_rows, long_rows and batches are osp_csr_mxm's of the same a and b whatever the
 * mask.  A SHORT row's products are tested against the mask as they are formed and only the survivors enter the sort in LDS
 * (a row that keeps few pays for a small sort); the products of the LONG rows are tested by a kernel that reads no value,
 * and only the survivors are expanded, sorted and folded.
 *
 * OSP_ERR_ARG: a null a, b, mask, sr or out; an add or mul outside osp_csr_mxm's lists; a non-zero reserved word in sr;
 * operands or a mask of different contexts; a and b of different dtypes; any of the three a result of osp_spgemm_partials;
 * any of the three with 2^32 - 1 entries or more.  OSP_ERR_DIM: a's N differs from b's M, or the mask's shape differs from
 * (a's M, b's N).  OSP_ERR_CAPACITY: as in osp_csr_mxm (ONE output row with 2^32 - 1 formed products or more).  On any
 * error *out and *stats are left as they were.
 *
 * M == 0, an empty a, an empty b, a product count of 0, an empty mask (not complemented: an empty result; complemented: the
 * bits of osp_csr_mxm) and a mask that admits nothing are legal and give an M x N result with a valid row pointer.  No
 * numeric kernel runs where nothing can be kept (no product, or an empty mask that is not complemented).
 *
 * stats (may be NULL): as commented in the struct.
 */
int osp_csr_mxm_masked(osp_result_t a, osp_result_t b, osp_result_t mask, int complement,
                       const osp_semiring_t *sr, osp_result_t *out, osp_mxm_masked_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MXM_MASKED_H */
