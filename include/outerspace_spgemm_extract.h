/*
 * outerspace_spgemm_extract.h -- the submatrix ("extract") of a CSR result on an AMD Instinct MI355X (gfx950):
 * out = in(rows, cols), renumbered, as a new CSR result, without leaving the device.
 *
 * Every other osp_csr_* function keeps the shape of its operand (the transpose turns it): osp_csr_select_vertices
 * (outerspace_spgemm_vector.h) removes vertices, but a removed vertex stays as an empty row and column.  This one renumbers:
 * a k-core, a cluster, a component or an ego network becomes a small matrix of its own, a batch of vertices gives its rows,
 * and a permutation reorders a matrix.  It adds ONE function and changes no existing struct (OSP_VERSION stays as
 * outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_EXTRACT_H
#define OUTERSPACE_SPGEMM_EXTRACT_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_extract {
    const uint32_t *rows;   /* NULL: every row of `in`, in order (n_rows ignored) */
    uint64_t        n_rows;
    const uint32_t *cols;   /* NULL: every column of `in` (n_cols ignored) */
    uint64_t        n_cols;
    int32_t         space;  /* osp_memspace_t of rows and cols */
    uint32_t        reserved[7];   /* must be 0 */
} osp_extract_t;

typedef struct osp_extract_stats {
    uint64_t nnz_in;         /* entries of `in` */
    uint64_t nnz_gathered;   /* entries of the gathered rows, before the column filter (rows NULL: nnz_in) */
    uint64_t nnz_out;        /* entries of `out` */
    float    ms_total;       /* device time of the call */
    uint32_t launches;       /* kernels launched, copies and memsets not counted */
    uint32_t readbacks;      /* blocking read-backs: see below */
    uint32_t reserved[5];    /* written 0 */
} osp_extract_stats_t;

/*
 * out(i, k) = in(rows[i], cols[k]) wherever `in` holds that entry.
 *   in -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   ex -- the two index lists, both in ex->space
 *
 * Shape.    out is an ordinary osp_result_t of n_rows x n_cols on in's context and of in's dtype, taken by every osp_result_*
 *           and osp_csr_* function, this one included.  Where a list is NULL that side is M or N and nothing is renumbered
 *           on it.
 * Rows.     Any order, duplicates allowed (a row of `in` taken k times is k rows of out), each below M.
 * Columns.  Strictly ascending, which also means without duplicates, and each below N.  Ascending columns are what keeps a
 *           row of out sorted without a sort; a permuted or repeating column list is built by composition with
 *           osp_csr_transpose (a row gather of the transpose; CsrResult.extract in Python does that).
 * Values.   Moved as integers of their width, never computed: NaN payloads, -0.0, denormals and explicit zeros survive.
 * Invariants.  Columns ascend in every row of out, row pointers are exact, and out is allocated at its exact size.
 * Result info.  osp_result_info(out) is in's with M = n_rows, N = n_cols, row_begin = 0, row_end = n_rows, nnz_c and
 *           ms_total replaced.
 * Empty lists.  A non-NULL list with a count of 0 is a legal empty list; its pointer is never dereferenced.  The result is
 *           0 x n or m x 0.
 * Both lists NULL.  out is a copy of in.
 *
 * Empty shapes.  When the counts alone say that out has no entry -- `in` has none, n_rows == 0 or n_cols == 0 -- nothing is
 * launched and neither list is read (so neither is checked).  When the gathered rows turn out to hold no entry, nothing is
 * launched after the read-back that says so.
 *
 * OSP_ERR_ARG: a null in, ex or out; a space outside osp_memspace_t; a non-zero reserved word; a result of
 * osp_spgemm_partials; an n_rows of 2^32 - 1 or more, or an n_cols above 2^32 - 1 (the limits of every result's shape); a row
 * index >= M; a column index >= N; columns that are not strictly ascending; an `in`, or gathered rows, of 2^32 - 1 entries or
 * more (the limit the other osp_csr_* functions put on their operand).  On any error *out and *stats are left as they
 * were.  That holds for lists in device memory too: the kernels that read a list never use an index beyond its dimension
 * as an address -- such a row has length 0, such a column sets no bit -- and raise a word that the call reads back before it
 * writes anything the index would have decided.
 *
 * Cost.  Work is cut by entries of the gathered rows, never by rows: one row of 2^20 entries taken three times and a
 * million short rows take the same path.  Per gathered entry one verdict bit is stored and nothing else: the gathered matrix
 * is never materialised.  The column list becomes a bitmap of N bits with one running count per 64 columns (12 bytes per
 * 64 columns), and the new index of a kept column is that count plus the population count of the bits below its own.  No
 * float atomics: the only atomic is the integer OR that fills the bitmap, whose result does not depend on any order.
 * Everything runs on the context's stream with temporary buffers from its pool.
 *
 * stats (may be NULL): nnz_in, nnz_gathered, nnz_out, ms_total as commented in the struct; launches = kernels launched
 * (copies and memsets not counted); readbacks = 0 for an empty shape and for a copy, 1 when either list is NULL or the
 * gathered rows hold no entry (the size of out, with the lists' error word), 2 otherwise (the gathered size with the error
 * word, then the size of out); reserved = 0.
 */
int osp_csr_extract(osp_result_t in, const osp_extract_t *ex, osp_result_t *out, osp_extract_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_EXTRACT_H */
