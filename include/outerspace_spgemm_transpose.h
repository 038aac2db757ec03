/*
 * outerspace_spgemm_transpose.h -- the transpose of a CSR result on an AMD Instinct MI355X (gfx950): out = in^T as a new CSR
 * result, without leaving the device.
 *
 * Every other osp_csr_* function keeps the orientation of its operand.  This one turns it: the CSR arrays of out are the CSC
 * arrays of in, so a result can be the LEFT operand of the outer-product pipeline (osp_spgemm_csc_csr takes A in CSC), and an
 * algorithm can walk the edges of a directed graph backwards.  It adds ONE function and changes no existing struct
 * (OSP_VERSION stays as outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_TRANSPOSE_H
#define OUTERSPACE_SPGEMM_TRANSPOSE_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_transpose {
    uint32_t reserved[8];   /* must be 0 */
} osp_transpose_t;

typedef struct osp_transpose_stats {
    uint64_t nnz;        /* entries of in = entries of out */
    uint32_t path;       /* 0: nothing launched, 1: row-mask path, 2: sort path */
    uint32_t passes;     /* radix passes of the sort path, else 0 */
    uint32_t launches;   /* kernels launched, copies and memsets not counted */
    float    ms_total;   /* device time of the call */
    uint32_t reserved[6];   /* written 0 */
} osp_transpose_stats_t;

/*
 * out = in^T.
 *   in -- any CSR result, M x N (not one of osp_spgemm_partials); it stays valid
 *   tp -- may be NULL; its reserved words must be 0
 *
 * out is N x M and has an entry (j, i) if and only if in has an entry (i, j); an explicit zero is an entry like any other.
 * Columns ascend in every row of out, row pointers are exact, and out is allocated at its exact size.  Values are moved as
 * integers of their width and never computed: NaN payloads, -0.0 and denormals survive, and transposing twice gives in back in
 * all three arrays.  out is an ordinary osp_result_t on in's context, taken by every osp_result_* and osp_csr_* function, this
 * one included.  osp_result_info(out): M = in's N, N = in's M, K = in's K, row_begin = 0, row_end = in's N,
 * nnz_a = nnz_c = the entries, nnz_b = 0, partials = 0, dtype in's, ms_total the call's time; every other field is 0.
 *
 * Two paths, chosen per call.  An in of at most 64 rows (a frontier, a batch of sources) takes the ROW-MASK path: one 64-bit
 * word per column collects the rows that hold it, the words' popcounts are out's row lengths, and an entry's place in its
 * output row is the popcount of the word below its row's bit.  Nothing is sorted.  Everything else takes the SORT path: a
 * stable radix sort of the entries by column with 8-bit digits, ceil(bits(N - 1) / 8) passes and at least one; the input is
 * in row order, so a stable sort leaves ascending rows inside every column.  Both paths give the same three arrays.
 * Environment, read per call: OSP_TRANSPOSE_PATH=sort takes the sort path whatever M is (any other value: automatic);
 * OSP_TRANSPOSE_GATHER=bisect lets the sort's last pass find an entry's row by a bisection of in's row pointer and fetch its
 * value separately, where the default packs (row, value) records before the sort and fetches one record per entry.
 *
 * OSP_ERR_ARG: a null in or out; a non-zero reserved word; a result of osp_spgemm_partials; an in of 2^32 - 1 entries or
 * more (the sort's positions are 32 bits); a non-empty in whose N is 2^32 - 256 or more (out's N + 1 row pointers are
 * written by one thread each in blocks of 256, and a launch takes fewer than 2^32 threads; refused before anything is launched
 * or allocated -- out's row pointers alone are 8 (N + 1) bytes).  OSP_ERR_DIM: in's M above 2^32 (a row index must fit a column).  On any error
 * *out and *stats are left as they were.  An in without entries (M == 0 and N == 0 included) is legal, launches nothing and
 * gives an empty N x M result.
 *
 * Everything runs on the context's stream with temporary buffers from its pool; there is no read-back (the size of out is
 * known).  No float atomics: the row-mask path's only atomic is an integer OR whose result does not depend on any order.
 *
 * stats (may be NULL): as commented in the struct.
 */
int osp_csr_transpose(osp_result_t in, const osp_transpose_t *tp /* may be NULL */, osp_result_t *out,
                      osp_transpose_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_TRANSPOSE_H */
