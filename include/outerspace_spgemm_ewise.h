/*
 * outerspace_spgemm_ewise.h -- the element-wise union and intersection of two CSR results on an AMD Instinct MI355X
 * (gfx950): combine, entry by entry, two CSR results that already exist, without leaving the device and without sorting
 * anything.
 *
 * osp_merge_csr_parts (outerspace_spgemm.h) sums parts that may be unsorted partial products and therefore sorts them;
 * the operands here are results, whose columns ascend in every row, so an entry's place in the output is found by a
 * search.  The union is the accumulation X <- X (+) Y of an iteration that sums a series of products and the
 * "visited += new" of a traversal; the intersection is the product of two results on their common pattern.  It adds ONE
 * function and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h, which this header includes, gives it).
 * No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_EWISE_H
#define OUTERSPACE_SPGEMM_EWISE_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSP_EWISE_UNION = 0,      /* pattern(a) | pattern(b) */
    OSP_EWISE_INTERSECT = 1   /* pattern(a) & pattern(b) */
} osp_ewise_mode_t;

typedef enum {
    OSP_EWISE_PLUS = 0,     /* a + b */
    OSP_EWISE_TIMES = 1,    /* a * b */
    OSP_EWISE_MIN = 2,      /* b < a ? b : a */
    OSP_EWISE_MAX = 3,      /* b > a ? b : a */
    OSP_EWISE_FIRST = 4,    /* a */
    OSP_EWISE_SECOND = 5,   /* b */
    OSP_EWISE_MINUS = 6,    /* a - b   (intersect only) */
    OSP_EWISE_DIV = 7       /* a / b   (intersect only) */
} osp_ewise_op_t;

typedef struct osp_ewise {
    int32_t  mode;          /* osp_ewise_mode_t */
    int32_t  op;            /* osp_ewise_op_t */
    uint32_t reserved[8];   /* must be 0 */
} osp_ewise_t;

typedef struct osp_ewise_stats {
    uint64_t nnz_a;         /* entries of `a` */
    uint64_t nnz_b;         /* entries of `b` */
    uint64_t nnz_both;      /* coordinates in both */
    uint64_t nnz_out;       /* entries of `out`: union nnz_a + nnz_b - nnz_both, intersect nnz_both */
    float    ms_total;      /* device time of the call */
    uint32_t launches;      /* kernels launched */
    uint32_t reserved[6];   /* written 0 */
} osp_ewise_stats_t;

/*
 * out = a (op) b, entry by entry.
 *   a, b  -- CSR results (not results of osp_spgemm_partials) of the same context, shape and dtype; both stay valid;
 *            a == b (the same handle) is legal
 *   ew    -- the mode and the operator
 *
 * UNION: out's pattern is pattern(a) | pattern(b).  A coordinate in both gets op(a, b); a coordinate in one operand only
 * keeps that operand's value bit for bit (NaN payloads and -0.0 included: it is copied, never computed).
 * INTERSECT: out's pattern is pattern(a) & pattern(b), and every value is op(a, b).
 *
 * op(a, b) is ONE IEEE operation in the results' dtype (the library is built without fast-math and with denormals on):
 * PLUS a + b, TIMES a * b, MINUS a - b, DIV a / b.  MIN is b < a ? b : a and MAX is b > a ? b : a: with a NaN in either
 * place the comparison is false and a is kept, and the result is always a copy of one operand's bits.  FIRST is a's bits,
 * SECOND b's bits.  Both modes are structural: an explicit zero is an entry like any other, and a computed zero
 * (x + (-x)) stays an entry.
 *
 * Under UNION, MINUS and DIV are OSP_ERR_ARG: an entry of b alone would be copied un-negated (un-inverted), which is not
 * a - b (a / b) with an absent a read as 0 (1) -- a trap and not a feature.  Negate or invert b first, or intersect.
 *
 * Columns ascend in every row, row pointers are exact, and out is allocated at its exact size.  out is an ordinary
 * osp_result_t on the operands' context, taken by every osp_result_* and osp_csr_* function, this one included.
 * osp_result_info(out) is a's with nnz_c and ms_total replaced (M, N and dtype are a's).
 *
 * OSP_ERR_ARG: a null a, b, ew or out; a mode or op outside its enum; MINUS or DIV under UNION; a non-zero reserved word;
 * operands of different contexts, shapes or dtypes; a result of osp_spgemm_partials; an operand of 2^32 - 1 entries or more
 * (positions inside a and b are kept in 32 bits, as osp_csr_apply_mask keeps its mask's).  On any error *out and *stats are
 * left as they were.  An empty a, an empty b and M == 0 are legal and launch no kernel: a union with an empty side is device
 * copies of the other side, an intersection with one is empty.
 *
 * Cost: nothing is sorted.  Union: b's entries are searched in a's rows (one bisection each), a's in b's; both operands
 * are read once more and out is written.  Intersect: a's entries are searched in b's rows, then the common ones are read
 * and written.  One read-back per call (nnz_both).  Everything runs on the context's stream with temporary buffers from
 * its pool; the work is cut by entries, so a few very long rows cost what many short ones cost, and no output position
 * depends on the order of processing.
 *
 * stats (may be NULL): nnz_a / nnz_b / nnz_both / nnz_out, ms_total = device time of the call, launches = kernels
 * launched (copies not counted), reserved = 0.
 */
int osp_csr_ewise(osp_result_t a, osp_result_t b, const osp_ewise_t *ew, osp_result_t *out, osp_ewise_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_EWISE_H */
