/*
 * outerspace_spgemm_assign.h -- the assignment of a CSR result INTO a region of another on an AMD Instinct MI355X (gfx950):
 * out = c with c(rows, cols) replaced by, or combined with, a -- as a new CSR result, without leaving the device
 * (DESIGN.md section 29).
 *
 * The inverse of osp_csr_extract (outerspace_spgemm_extract.h): a block update of a result, the embedding of a small result
 * in a larger index space, the assembly of a block matrix, a processed subgraph put back where it was cut out.  It adds ONE
 * function and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h, which this header includes through
 * outerspace_spgemm_ewise.h, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_ASSIGN_H
#define OUTERSPACE_SPGEMM_ASSIGN_H

#include "outerspace_spgemm_ewise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSP_ASSIGN_NO_ACCUM (-1)

typedef struct osp_assign {
    const uint32_t *rows;   /* NULL: row i of a goes to row i of c (a must have c's M rows; n_rows ignored) */
    uint64_t        n_rows;
    const uint32_t *cols;   /* NULL: column k of a goes to column k of c (a must have c's N columns; n_cols ignored) */
    uint64_t        n_cols;
    int32_t         space;  /* osp_memspace_t of rows and cols */
    int32_t         accum;  /* OSP_ASSIGN_NO_ACCUM, or an osp_ewise_op_t from PLUS to SECOND */
    uint32_t        reserved[6];   /* must be 0 */
} osp_assign_t;

typedef struct osp_assign_stats {
    uint64_t nnz_c, nnz_a;   /* entries of the operands */
    uint64_t nnz_region;     /* entries of c inside rows x cols */
    uint64_t nnz_both;       /* coordinates of the region held by c and by a */
    uint64_t nnz_out;        /* entries of out */
    float    ms_total;       /* device time of the call */
    uint32_t launches;       /* kernels launched; copies and memsets not counted */
    uint32_t readbacks;      /* blocking read-backs: see below */
    uint32_t reserved[5];    /* written 0 */
} osp_assign_stats_t;

/*
 * out = c, except inside the region rows x cols, where a's entry (i, k) stands at (rows[i], cols[k]).
 *   c  -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   a  -- a CSR result of m x n on c's context and of c's dtype, m = n_rows (M when rows is NULL), n = n_cols (N when cols
 *         is NULL); it stays valid.  a == c is legal where the shapes allow it.
 *   as -- the two index lists, both in as->space, and the accum operator
 *
 * Result.   out is a NEW ordinary osp_result_t of M x N, taken by every osp_result_* and osp_csr_* function, this one
 *           included: exact row pointers, ascending columns in every row, allocated at its exact size.
 *           osp_result_info(out) is c's with nnz_c and ms_total replaced.
 * Outside the region.  c's entries, bit for bit.
 * Inside, without accum (OSP_ASSIGN_NO_ACCUM).  GrB_assign's replacement of the region: a(i, k) where a holds it, otherwise
 *           NOTHING -- an entry of c inside the region that a does not hold is deleted.
 * Inside, with accum op.  op(c, a) where both hold the coordinate, c first; where only one holds it, that one's value, bit
 *           for bit; absent where neither does.  SECOND is therefore not "no accum": it keeps c's entries that a lacks.
 *           op is one IEEE operation in the dtype, or a copy of one operand's bits, exactly as in osp_csr_ewise.  MINUS and
 *           DIV are refused, as under the union: an entry of a alone would be copied as it is.
 * Values.   Everything that is not computed is moved as integers of its width: NaN payloads, -0.0, denormals and explicit
 *           zeros survive.  A computed zero stays an entry.
 * Rows.     Any order, each below M, DISTINCT (a repeated row has no defined meaning in GraphBLAS either).
 * Columns.  Strictly ascending, each below N, as in osp_csr_extract: that keeps a row of out sorted without a sort.  A
 *           permuted column list is handled by composition with osp_csr_extract (CsrResult.assign in Python does that).
 * Empty lists.  A non-NULL list with a count of 0 is a legal empty list; its pointer is never dereferenced.
 *
 * No-work shapes.  These launch nothing and read no list (so check none): M == 0 (out is empty); m == 0 or n == 0 (a copy of
 * c); both lists NULL without accum (a copy of a); c and a both without entries; with accum, an a without entries (a copy of
 * c).  They report launches == 0, readbacks == 0, nnz_region == 0 and nnz_both == 0 (neither was counted).
 * Everything else takes the general path: a c without entries and an a with some is the embedding of a, an a without
 * entries and no accum only deletes the region, both lists NULL with accum is the union.
 *
 * OSP_ERR_DIM: a's shape is not (m, n).
 * OSP_ERR_ARG: a null c, a, as or out; a space outside osp_memspace_t; an accum that is neither OSP_ASSIGN_NO_ACCUM nor
 * one of PLUS .. SECOND; a non-zero reserved word; a result of osp_spgemm_partials; operands of different contexts or
 * dtypes; an n_rows of 2^32 - 1 or more, or an n_cols above 2^32 - 1 (the limits of every result's shape); a row index
 * >= M; a repeated row index; a column index >= N; columns that are not strictly ascending; an operand of 2^32 - 1 entries
 * or more; on the general path, a c of more than 2^32 - 256 rows.  The argument checks come before the shape check.
 * On any error *out and *stats are left as they were.  That holds for lists in device memory too: the kernels that read a
 * list never use an index beyond its dimension as an address -- such a row claims no word of the row map, such a column
 * sets no bit -- and raise a word that the call reads back before it writes anything of out.
 *
 * Cost.  Work is cut by entries, never by rows: one pass over c's columns that stores one bit per entry ("c's side does not
 * write this entry"), then one pass that moves c's kept entries and one that moves a's, each entry to a position that is a
 * function of that bit array, its scan and a bisection in the other operand's row.  The matrix "a embedded in M x N" is never
 * stored and no intermediate CSR is written.  The row list becomes M 32-bit words, the column list the bitmap of
 * osp_csr_extract (12 bytes per 64 columns).  No sort, no float atomics: the atomics are integer ones (the claim of a row's
 * word, the OR that fills the bitmap, one counter) whose results do not depend on any order.  Everything runs on the
 * context's stream with temporary buffers from its pool.
 *
 * stats (may be NULL): as commented in the struct; readbacks = 0 for a no-work shape, 1 otherwise (the lists' error word
 * together with the two counts that size out); reserved = 0.
 */
int osp_csr_assign(osp_result_t c, osp_result_t a, const osp_assign_t *as, osp_result_t *out, osp_assign_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_ASSIGN_H */
