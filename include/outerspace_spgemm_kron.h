/*
 * outerspace_spgemm_kron.h -- the Kronecker product of two CSR results on an AMD Instinct MI355X (gfx950):
 * out = a (x) b -- as a new CSR result, without leaving the device.
 *
 * GrB_kronecker: Kronecker graphs (the deterministic model behind R-MAT, whose triangle count, degrees and nnz are known in
 * closed form from the seed), the tensor, Cartesian and strong products of two graphs, and block structure (I (x) b is the
 * disjoint union of copies of b, J (x) b replicates a block).  It adds ONE function and changes no existing struct
 * (OSP_VERSION stays as outerspace_spgemm.h, which this header includes through outerspace_spgemm_ewise.h, gives it).  No
 * reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_KRON_H
#define OUTERSPACE_SPGEMM_KRON_H

#include "outerspace_spgemm_ewise.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kernels of a call that has work to do: the row pointers and the entries (a no-work shape launches none) */
#define OSP_KRON_LAUNCHES 2

typedef struct osp_kron {
    int32_t  op;            /* an osp_ewise_op_t: TIMES, PLUS, MIN, MAX, FIRST or SECOND */
    uint32_t reserved[7];   /* must be 0 */
} osp_kron_t;

typedef struct osp_kron_stats {
    uint64_t nnz_a, nnz_b;   /* entries of the operands */
    uint64_t nnz_out;        /* entries of out: nnz_a * nnz_b */
    float    ms_total;       /* device time of the call */
    uint32_t launches;       /* kernels launched; copies and memsets not counted */
    uint32_t readbacks;      /* blocking read-backs: 0 on every path */
    uint32_t reserved[5];    /* written 0 */
} osp_kron_stats_t;

/*
 * out = a (x) b: with a of mA x nA and b of mB x nB, out is (mA mB) x (nA nB), and for every entry (ia, ja) of a and every
 * entry (ib, jb) of b it holds op(a(ia, ja), b(ib, jb)) at (ia mB + ib, ja nB + jb), a's value first.
 *   a, b -- CSR results on one context and of one dtype (not results of osp_spgemm_partials); both stay valid.  a == b (the
 *           same handle) is legal.
 *   kr   -- the operator
 *
 * Result.   out is a NEW ordinary osp_result_t, taken by every osp_result_* and osp_csr_* function, this one included:
 *           exact row pointers, ascending columns in every row, allocated at its exact size.
 *           osp_result_info(out): M = mA mB, K = 0, N = nA nB, row_begin = 0, row_end = M, nnz_a, nnz_b, nnz_c, partials =
 *           nnz_c, dtype, ms_total; every other field is 0.
 * Operator. op is one of the mul operators of osp_semiring_t: one IEEE operation in the dtype (TIMES, PLUS) or a copy of one
 *           operand's bits (MIN, MAX, FIRST, SECOND), exactly as in osp_csr_ewise.  Values that are not computed are moved
 *           as integers of their width: NaN payloads, -0.0 and denormals survive.  MINUS and DIV are refused.
 * Structure.  The product is structural: an explicit zero of an operand makes entries, and a computed zero stays an entry.
 *
 * Closed form.  With rpA, rpB the operands' row pointers and lenA[i] = rpA[i + 1] - rpA[i]:
 *           row r = ia mB + ib of out begins at rpA[ia] nnzB + lenA[ia] rpB[ib] and holds lenA[ia] lenB[ib] entries; its
 *           q-th entry comes from a's entry rpA[ia] + q / lenB[ib] and b's entry rpB[ib] + q % lenB[ib], and its column is
 *           colA nB + colB, which ascends with q.  Nothing is sorted, scanned or counted.
 *
 * No-work shapes.  An operand without entries, or M == 0, gives the empty M x N result; it launches nothing and reports
 * launches == 0.
 *
 * OSP_ERR_ARG: a null a, b, kr or out; an op outside the six (MINUS, DIV and out-of-range values included); a non-zero
 * reserved word; operands of different contexts or dtypes; a result of osp_spgemm_partials; an operand of 2^32 - 1 entries
 * or more; mA mB >= 2^32 - 1 or nA nB > 2^32 - 1 (the limits of every result's shape, computed in 64 bits).
 * OSP_ERR_CAPACITY: nnzA nnzB >= 2^32 - 1 -- no other operation would take such a result as an operand, and the cap keeps
 * every offset inside a row of out in 32 bits.  The legal maximum of 2^32 - 2 entries is 51 GB in f64: it is NOT tested.
 * The argument checks come before the size checks.  On any error *out and *stats are left as they were.
 *
 * Cost.  Work is cut by OUTPUT positions, never by rows of either operand: a hub row (x) a hub row is one row of out of
 * millions of entries, an operand with a few entries in 2^20 rows makes millions of empty ones, and both take the same path
 * at the same cost per entry.  OSP_KRON_LAUNCHES kernels on the general path: one lane per row of out evaluates the row
 * pointer's closed form; then every lane owns a few consecutive output positions, finds the first one's (ia, ib) by
 * bisection of the two row pointers, steps to the others, and stores columns and values 16 bytes at a time.  No atomics, no
 * temporary memory -- the only allocations are out's three arrays -- and no read-back: the host knows nnzA nnzB.
 *
 * stats (may be NULL): as commented in the struct; launches = OSP_KRON_LAUNCHES, or 0 for a no-work shape; readbacks = 0;
 * reserved = 0.
 */
int osp_csr_kron(osp_result_t a, osp_result_t b, const osp_kron_t *kr, osp_result_t *out, osp_kron_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_KRON_H */
