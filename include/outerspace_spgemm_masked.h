/*
 * outerspace_spgemm_masked.h -- the masked product C<M> = A*B on an AMD Instinct MI355X (gfx950).
 *
 * A family of its own beside the outer-product pipeline of outerspace_spgemm.h (which it includes): every output entry is
 * the intersection of a row of A with a column of B, summed in ascending k.  No reference
 * counterpart; the reference's finetune masks its gradients this way on the host (NN_models/main.py).
 */
#ifndef OUTERSPACE_SPGEMM_MASKED_H
#define OUTERSPACE_SPGEMM_MASKED_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * C (MxN, CSR) = A (MxK, CSC) * B (KxN, CSR), restricted to the pattern of the mask M (MxN, CSR, pattern only).
 *   a_colptr[K+1], a_rowidx[nnzA], a_vals[nnzA]   -- as osp_spgemm_csc_csr
 *   b_rowptr[K+1], b_colidx[nnzB], b_vals[nnzB]   -- as osp_spgemm_csc_csr
 *   m_rowptr[M+1], m_colidx[nnzM]                 -- the mask; it has no values
 * `space` says where ALL eight arrays live.  cfg may be NULL (defaults).
 *
 * C has an entry at (i, j) if and only if (i, j) is in the mask and at least one k has a stored A[i,k] and a stored
 * B[k,j].  This is structural: explicit zeros count, and a sum that cancels to 0 is kept.  So C is the unmasked product
 * with every entry outside the mask removed -- the same row pointers, columns and value bits (every entry summed left to
 * right in ascending k, without contraction, as osp_spgemm_csc_csr sums it).  Columns ascend in every row.
 *
 * cfg: `validate` checks A and B as osp_spgemm_csc_csr does, and the mask: a monotone 0..nnzM rowptr (OSP_ERR_ARG),
 * columns < N (OSP_ERR_RANGE), ascending columns (OSP_ERR_UNSORTED) and no duplicates (OSP_ERR_DUPLICATE, 233); without
 * it a violation indexes out of bounds on the device.  k_begin / k_end must be 0 / 0 and row_shard_count <= 1, anything
 * else is OSP_ERR_ARG.  partial_capacity and algorithm are ignored.
 * Limits: nnzA, nnzB and nnzM must each be below 2^32 (OSP_ERR_ARG).  A null m_rowptr, or a null m_colidx with nnzM > 0,
 * is OSP_ERR_ARG.  M, K and N must each be below 2^32 - 256 (osp_spgemm_csc_csr takes N up to 2^32 - 1), or the call is
 * refused with OSP_ERR_ARG before anything is launched or allocated: the call makes a column view of B with N + 1 offsets (and
 * a row view of A with M + 1), one thread each in blocks of 256, and a launch takes fewer than 2^32 threads.  Its device footprint is therefore 8 (N + 1) bytes beside
 * the operands', whatever they hold (16 GiB at N = 2^31).  On any error *result is left as it was.
 *
 * The result is an ordinary osp_result_t: osp_result_copy_csr, _device_ptrs, _info, _write_mtx, _coo_rows,
 * osp_csr_bias_relu and osp_result_destroy all take it.  osp_result_info fills these fields of osp_result_info_t:
 *   M, K, N              the shapes of the call
 *   row_begin, row_end   0 and M
 *   nnz_a, nnz_b, nnz_c  entries of A, B and C
 *   partials             the number of products formed: the sum over mask entries (i, j) of |{k : A[i,k], B[k,j] stored}|
 *                        (NOT the unmasked product's P = sum_k nnz(A[:,k]) * nnz(B[k,:]))
 *   dtype                as given
 *   ms_total             device time of the whole call, host copies included
 *   ms_ingest            the two operand transposes (A to row order, B to column order), included in ms_total
 *   ms_multiply_kernel   the intersection kernels, included in ms_total
 *   multiply_launches    the number of intersection kernel launches (0, 1 or 2: light slots, heavy slots)
 * Every other field is 0.
 */
int osp_spgemm_masked(osp_context_t ctx, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N,
                      const int64_t *a_colptr, const uint32_t *a_rowidx, const void *a_vals,
                      const int64_t *b_rowptr, const uint32_t *b_colidx, const void *b_vals,
                      const int64_t *m_rowptr, const uint32_t *m_colidx,
                      osp_memspace_t space, const osp_config_t *cfg, osp_result_t *result);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MASKED_H */
