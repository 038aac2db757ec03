/*
 * outerspace_spgemm_apply_mask.h -- the mask filter C<M> / C<¬M> on an AMD Instinct MI355X (gfx950): keep, of a CSR result
 * that already exists, the entries a pattern names -- or the entries it does not name -- without leaving the device
 * (DESIGN.md section 11).
 *
 * osp_spgemm_masked (outerspace_spgemm_masked.h) computes a product AT a pattern; this header is the other half of masking,
 * the complemented mask included.  It is the step between two products of a traversal: a level of breadth-first search is
 * next<¬visited> = frontier * Adj.  It adds ONE function and changes no existing struct (OSP_VERSION stays as
 * outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_APPLY_MASK_H
#define OUTERSPACE_SPGEMM_APPLY_MASK_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_apply_mask_stats {
    uint64_t nnz_in;        /* entries of `in` */
    uint64_t nnz_mask;      /* entries of the mask */
    uint64_t nnz_out;       /* entries of `out` */
    float    ms_total;      /* device time of the call, the host copies of a host mask included */
    uint32_t launches;      /* kernels launched */
    uint32_t reserved[6];   /* written 0 */
} osp_apply_mask_stats_t;

/*
 * out = in<mask> (complement == 0) or in<¬mask> (complement != 0).
 *   in                              -- any CSR result (not one of osp_spgemm_partials); it stays valid
 *   M, N                            -- the mask's shape; must equal in's (OSP_ERR_ARG)
 *   m_rowptr[M+1], m_colidx[nnzM]   -- the mask, an MxN CSR PATTERN (it has no values), both arrays in `space`: the arrays
 *                                      osp_spgemm_masked takes for its mask
 *
 * complement == 0: out holds the entries (i, j) of `in` that ARE in the mask; complement != 0: those that are NOT.  This is
 * structural on both sides: an explicit zero of `in` is an entry like any other, and the mask has no values.  For every
 * `in` and mask the two senses partition `in`.
 *
 * A kept entry keeps its value bit for bit (NaN payloads and -0.0 included: values are copied, never computed).  Columns
 * stay ascending in every row, row pointers are exact, and out is allocated at its exact size.  out is an ordinary
 * osp_result_t on in's context, taken by every osp_result_* function, osp_csr_bias_relu, osp_csr_inflate_prune and
 * osp_csr_apply_mask itself.  osp_result_info(out) is in's with nnz_c and ms_total replaced (M, N and dtype are in's).
 *
 * validate != 0 checks the mask as osp_spgemm_masked does: a monotone 0..nnzM rowptr (OSP_ERR_ARG), columns < N
 * (OSP_ERR_RANGE), ascending columns (OSP_ERR_UNSORTED) and no duplicates (OSP_ERR_DUPLICATE, 233).  Without it the result
 * for a mask with unsorted or duplicate columns is unspecified (no access leaves the arrays the row pointers delimit); row
 * pointers that are not a monotone 0..nnzM sequence index out of bounds on the device.
 * A null in, out or m_rowptr, a null m_colidx with nnzM > 0, nnzM >= 2^32, a bad `space`, a result of osp_spgemm_partials
 * and a shape other than in's are OSP_ERR_ARG.  On any error *out and *stats are left as they were.
 *
 * Zero-sized cases are legal: an empty `in`, an empty mask, M == 0.  They launch no filter kernel (an empty mask in the
 * complement sense is three device copies).
 *
 * Cost: `in` is read once for its columns and once more for the kept entries; one read-back per call (nnz_out; the nnzM of
 * a device mask comes back with it); validate != 0 adds one per validation kernel, and the nnzM of a device mask is read up
 * front when validate != 0, when m_colidx is null or when `in` is empty.  Everything runs on the context's stream with temporary buffers from its pool; the work is cut by
 * entries of `in`, so a few very long rows cost what many short ones cost.
 *
 * stats (may be NULL): nnz_in / nnz_mask / nnz_out, ms_total = device time of the call (host copies of a host mask
 * included), launches = kernels launched (copies not counted), reserved = 0.
 */
int osp_csr_apply_mask(osp_result_t in, uint64_t M, uint64_t N,
                       const int64_t *m_rowptr, const uint32_t *m_colidx, osp_memspace_t space,
                       int complement, int validate,
                       osp_result_t *out, osp_apply_mask_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_APPLY_MASK_H */
