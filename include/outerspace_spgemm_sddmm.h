/*
 * outerspace_spgemm_sddmm.h -- the sampled dense-dense product on an AMD Instinct MI355X (gfx950): dense X (M x k) times
 * dense Y^T (k x N) under a named semiring, evaluated ONLY where a CSR result has entries, without leaving the device
 * (DESIGN.md section 23):
 *
 *     out(i, j) = accum(in(i, j), R_add over c of mul(X[i, c], Y[j, c]))      for the entries (i, j) of `in`
 *
 * The other half of osp_csr_mxd (outerspace_spgemm_mxd.h, which this header includes for osp_semiring_t and
 * OSP_MXD_MAX_COLS): attention and edge scores of a graph neural network, the gradient of osp_csr_mxd with respect to its
 * sparse operand, link-prediction scores of an edge list, the residual of a factorisation on its observed entries, and under
 * (MIN, PLUS) the landmark bound min_c d(c, u) + d(c, v) of a list of vertex pairs.  It adds ONE function and changes no
 * existing struct (OSP_VERSION stays as outerspace_spgemm.h gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_SDDMM_H
#define OUTERSPACE_SPGEMM_SDDMM_H

#include "outerspace_spgemm_mxd.h"
#include "outerspace_spgemm_vector.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_sddmm_stats {
    uint64_t nnz_in;           /* entries of `in` */
    uint64_t nnz_out;          /* entries of `out`: the same number */
    uint64_t cols;             /* k */
    uint32_t lanes_per_entry;  /* lanes an entry gets in a wave: the power of two >= min(k, 64); 64 / lanes_per_entry entries per batch */
    uint32_t launches;         /* kernels launched, copies not counted */
    float    ms_total;         /* device time of the call */
    uint32_t reserved[7];      /* written 0 */
} osp_sddmm_stats_t;

/*
 * out = a new result with in's pattern; at (i, j) its value is accum(c, d) with c = in's value there and
 * d = R_add(p_0 .. p_{k-1}), p_c = mul(x[i, c], y[j, c]).
 *   in    -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   sr    -- osp_csr_mxv's operators: add is PLUS, MIN or MAX; mul is TIMES, PLUS, MIN, MAX, FIRST or SECOND; the reserved
 *            words must be 0
 *   accum -- osp_csr_apply_vectors' operators, in its operand order: PLUS c + d, TIMES c * d, MINUS c - d, DIV c / d, MIN,
 *            MAX, SECOND d; OSP_VECTOR_NONE means SECOND.  SECOND and NONE load no value of `in`.  FIRST is refused: it
 *            would be a copy of `in`.
 *   x     -- M x k values of in's dtype in `space`, row-major, contiguous (x[i, c] at i * k + c); may be NULL when mul is
 *            SECOND
 *   y     -- N x k values, likewise; may be NULL when mul is FIRST; x == y is legal
 *   k     -- the length of the reduction, at most OSP_MXD_MAX_COLS
 *
 * The result is DEFINED TO THE BIT, with no tolerance.  R, its identities (+0.0 for PLUS, +inf for MIN, -inf for MAX) and
 * (+) are exactly those of osp_csr_reduce (outerspace_spgemm_vector.h): 64 lane partials filled left to right with stride
 * 64, the butterfly d = 32 .. 1, and for k > 2048 R over the R of the consecutive blocks of 2048.  mul is the one IEEE
 * operation or copy of osp_csr_ewise, x's element in a's place; a product and the addition after it are two roundings:
 * nothing is contracted.  Equivalently: take the one-row CSR that holds x[i, 0..k) at the columns 0..k-1; d at (i, j) equals
 * osp_csr_mxv of that CSR with the vector y[j, :], bit for bit.
 *
 * k == 0 is legal (d is the identity).  An `in` without entries (M == 0 and N == 0 included) is legal and launches nothing,
 * and reads neither x nor y: out is an empty M x N result.  out's rowptr and colidx are copies of in's.
 *
 * A call that fails leaves *out and *stats as they were.  OSP_ERR_ARG: a null in, sr or out; a null x or y that mul needs;
 * an operator outside its list; a non-zero reserved word; a bad space; a result of osp_spgemm_partials;
 * k > OSP_MXD_MAX_COLS.
 *
 * Everything runs on the context's stream with temporary buffers from its pool (host-space x and y are staged there); work
 * is cut by entries, 64 to a wave, so a row of any length costs what its entries cost; no LDS, no atomics, no waiting
 * between workgroups, no read-back.
 *
 * stats (may be NULL): as commented in the struct.  launches is 1 when `in` has entries and 0 otherwise.
 */
int osp_csr_sddmm(osp_result_t in, const osp_semiring_t *sr, int accum /* osp_ewise_op_t or OSP_VECTOR_NONE */,
                  const void *x, const void *y, uint64_t k, osp_memspace_t space,
                  osp_result_t *out, osp_sddmm_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_SDDMM_H */
