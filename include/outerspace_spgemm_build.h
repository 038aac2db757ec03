/*
 * outerspace_spgemm_build.h -- a CSR result built from a COO list on an AMD Instinct MI355X (gfx950): the list may come in any
 * order and may name a coordinate more than once; the repeats are combined by a named operator in LIST order (DESIGN.md
 * section 19).  GraphBLAS calls it GrB_Matrix_build.
 *
 * Every osp_csr_* function takes a result that exists already; osp_spgemm_coo sorts COO lists on the device, but only as the
 * operands of a product, and refuses a repeated coordinate.  This is the way in: an edge list becomes an adjacency matrix, a
 * multigraph's list a weighted graph, a Laplacian or an incidence matrix, in one call.  It adds ONE function and changes no
 * existing struct (OSP_VERSION stays as outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_BUILD_H
#define OUTERSPACE_SPGEMM_BUILD_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSP_DUP_ERROR = 0,   /* a repeated coordinate fails the call with OSP_ERR_DUPLICATE */
    OSP_DUP_PLUS,        /* acc + v */
    OSP_DUP_MIN,         /* v < acc ? v : acc */
    OSP_DUP_MAX,         /* v > acc ? v : acc */
    OSP_DUP_FIRST,       /* the first of the list */
    OSP_DUP_LAST,        /* the last of the list */
    OSP_DUP_COUNT        /* how many the list holds, as a value */
} osp_dup_op_t;

typedef struct osp_build {
    uint64_t M, N, nnz;            /* the result's shape, the list's length */
    const uint32_t *rows, *cols;   /* nnz each */
    const void *vals;              /* nnz values of dtype; NULL: every value is 1 */
    int32_t dtype, space, dup;     /* osp_dtype_t, osp_memspace_t (all three arrays), osp_dup_op_t */
    uint32_t reserved[7];          /* must be 0 */
} osp_build_t;

typedef struct osp_build_stats {
    uint64_t nnz_in;      /* entries of the list */
    uint64_t nnz_out;     /* entries of `out`: the distinct coordinates */
    uint64_t long_runs;   /* runs folded by a whole wave: see Cost */
    float    ms_total;    /* device time of the call */
    uint32_t launches;    /* kernels launched, copies and memsets not counted */
    uint32_t readbacks;   /* blocking read-backs: see below */
    uint32_t reserved[5]; /* written 0 */
} osp_build_stats_t;

/*
 * out(r, c) = the combination of every list entry (rows[t], cols[t], vals[t]) with that coordinate.
 *   ctx -- the context `out` lives on
 *   b   -- the shape, the list (all three arrays in b->space) and the operator
 *
 * Shape.    out is an ordinary osp_result_t of M x N on ctx and of b->dtype, taken by every osp_result_* and osp_csr_*
 *           function.
 * Invariants.  Columns ascend strictly in every row of out, row pointers are exact, and out is allocated at its exact size.
 * Result info.  osp_result_info(out) holds M, N, row_begin = 0, row_end = M, nnz_c, ms_total, dtype and the context's two
 *           variant words; every other field is 0 (what osp_csr_extract leaves of an imported result's).
 *
 * Runs.     A RUN is the set of list entries with one coordinate (r, c), in LIST order: e_0 ... e_{m-1}, their positions t in
 *           the list ascending.  The result depends on the list alone -- on each run's values in list order -- and not on
 *           where a run falls in any internal array, on the order of other runs, or on the path that folds it.
 * m == 1.   The value's bits are moved, never computed: NaN payloads, -0.0, denormals and explicit zeros survive (COUNT
 *           excepted: it reads no value).
 * m >= 2.   acc = e_0, then acc = acc (+) e_t for t = 1 ... m - 1, strictly in that order, (+) being
 *             OSP_DUP_PLUS   acc + v, ONE IEEE addition in dtype
 *             OSP_DUP_MIN    v < acc ? v : acc     (osp_csr_ewise's expressions: a NaN never replaces acc, a NaN acc is never
 *             OSP_DUP_MAX    v > acc ? v : acc      replaced; of -0.0 and +0.0 the earlier stays; what moves is bits)
 *             OSP_DUP_FIRST  e_0's bits
 *             OSP_DUP_LAST   e_{m-1}'s bits
 *             OSP_DUP_COUNT  (T)m, also for m == 1; no value is read, vals may be anything
 *             OSP_DUP_ERROR  the call fails with OSP_ERR_DUPLICATE (233)
 * vals NULL.  Every value is 1: PLUS gives what the chain 1 + 1 + ... gives in dtype (m, and in f32 2^24 from m = 2^24 on),
 *           MIN, MAX, FIRST and LAST give 1, COUNT gives (T)m.  Nothing is gathered.
 *
 * Empty shapes.  nnz == 0, M == 0 or N == 0 launches nothing and reads no list (so the list is not checked): out is M x N
 * without entries.
 *
 * OSP_ERR_ARG: a null ctx, b or out; null rows or cols with nnz > 0; a dtype outside osp_dtype_t, a space outside
 * osp_memspace_t, a dup outside osp_dup_op_t; a non-zero reserved word; M of 2^32 - 1 or more or N above 2^32 - 1 (the limits
 * of every result's shape); nnz of 2^32 - 1 or more.
 * OSP_ERR_RANGE: a row >= M or a column >= N (checked before duplicates: a list with both fails with OSP_ERR_RANGE).
 * OSP_ERR_DUPLICATE: OSP_DUP_ERROR and a coordinate given twice.
 * On any error *out and *stats are left as they were.  That holds for lists in device memory too: an index beyond its
 * dimension is only ever a sort key, never an address, and raises an error word that comes back with the read-back of
 * nnz_out, before out is allocated.
 *
 * Cost.  Two stable radix sorts (by column, then by row: the sorts osp_spgemm_coo uses) leave every run contiguous and in
 * list order; they bound the call from below.  After them work is cut by sorted ENTRIES, 2048 a workgroup, never by rows or
 * by runs.  One bit per entry says whether it begins a run; the scan of the words' population counts gives every run its place
 * and nnz_out.  Only a run's first entry works: its length is the distance to the next set bit, its values are gathered from
 * the caller's array through the sort's permutation -- and ONLY those the operator needs: one per run for FIRST and LAST, none
 * for COUNT or with vals NULL.  A run of up to 64 entries is folded by its lane; a longer one under PLUS, MIN or MAX (with
 * values) by its whole wave, 64 values loaded at once and then combined in order, and counted in long_runs (0 for the other
 * operators and with vals NULL).  No float atomics and no waiting between workgroups: the only atomics are the integer OR of
 * the error word and the integer count of long_runs, whose results do not depend on order.  Everything runs on the context's
 * stream with temporary buffers from its pool.
 *
 * stats (may be NULL): nnz_in, nnz_out, long_runs, ms_total as commented in the struct; launches = kernels launched (copies
 * and memsets not counted); readbacks = 0 for an empty shape, 1 when no coordinate repeats or the operator folds nothing by
 * a wave (FIRST, LAST, COUNT, ERROR, vals NULL): nnz_out with the error word, 2 otherwise: then also long_runs, after the
 * last kernel; reserved = 0.
 */
int osp_csr_build(osp_context_t ctx, const osp_build_t *b, osp_result_t *out, osp_build_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_BUILD_H */
