/*
 * outerspace_spgemm_select.h -- the entry filter ("select") of a CSR result on an AMD Instinct MI355X (gfx950): keep, of a
 * CSR result that already exists, the entries whose VALUE passes a comparison with a threshold, or whose POSITION lies on one
 * side of a diagonal, without leaving the device.
 *
 * osp_csr_apply_mask (outerspace_spgemm_apply_mask.h) filters by a pattern; this header filters by the entry itself, and can
 * write a constant in place of the kept values.  That is the step between two support products of a k-truss:
 * A = pattern of S where S >= k - 2, values reset to 1.  It adds ONE function and changes no existing struct (OSP_VERSION
 * stays as outerspace_spgemm.h, which this header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_SELECT_H
#define OUTERSPACE_SPGEMM_SELECT_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSP_SELECT_LT = 0,       /* value <  threshold */
    OSP_SELECT_LE = 1,       /* value <= threshold */
    OSP_SELECT_GT = 2,       /* value >  threshold */
    OSP_SELECT_GE = 3,       /* value >= threshold */
    OSP_SELECT_EQ = 4,       /* value == threshold */
    OSP_SELECT_NE = 5,       /* value != threshold */
    OSP_SELECT_TRIL = 6,     /* col <= row + diag */
    OSP_SELECT_TRIU = 7,     /* col >= row + diag */
    OSP_SELECT_DIAG = 8,     /* col == row + diag */
    OSP_SELECT_OFFDIAG = 9   /* col != row + diag */
} osp_select_op_t;

typedef struct osp_select {
    int32_t  op;            /* osp_select_op_t */
    int32_t  fill;          /* 0: kept entries keep their values; != 0: every kept entry's value is fill_value */
    double   threshold;     /* value predicates */
    int64_t  diag;          /* position predicates */
    double   fill_value;    /* fill != 0: rounded to the result's dtype (beyond its largest number: the infinity of that sign) */
    uint32_t reserved[8];   /* must be 0 */
} osp_select_t;

typedef struct osp_select_stats {
    uint64_t nnz_in;        /* entries of `in` */
    uint64_t nnz_out;       /* entries of `out` */
    float    ms_total;      /* device time of the call */
    uint32_t launches;      /* kernels launched */
    uint32_t reserved[6];   /* written 0 */
} osp_select_stats_t;

/*
 * out = the entries of `in` that pass sel->op.
 *   in    -- any CSR result (not one of osp_spgemm_partials); it stays valid
 *   sel   -- the predicate and what is written for a kept entry
 *
 * Value predicates (LT .. NE) compare the stored value, widened exactly to double for an f32 result, with sel->threshold
 * under IEEE rules: every comparison with a NaN on either side is false except NE, which is true; -0.0 == +0.0; infinities
 * and denormals compare as the numbers they are.  Position predicates (TRIL .. OFFDIAG) compare the entry's column with
 * row + sel->diag as signed 64-bit integers, on any shape (M != N included) and for a diag of either sign, beyond the matrix
 * included.  Both kinds are structural: an explicit zero of `in` is an entry like any other.
 * For every `in`: EQ and NE partition it; LT and GE partition it when it holds no NaN; TRIL(d) and TRIU(d + 1) partition it;
 * DIAG(d) and OFFDIAG(d) partition it.
 *
 * fill == 0: a kept entry keeps its value bit for bit (NaN payloads and -0.0 included: values are copied, never computed).
 * fill != 0: every kept entry's value is fill_value rounded to the result's dtype (a magnitude beyond the dtype's largest
 * number becomes the infinity of its sign), and in's values are not read when the output is written (a position predicate
 * with fill never reads them at all).
 *
 * Columns stay ascending in every row, row pointers are exact, and out is allocated at its exact size.  out is an ordinary
 * osp_result_t on in's context, taken by every osp_result_* function, osp_csr_bias_relu, osp_csr_inflate_prune,
 * osp_csr_apply_mask and osp_csr_select itself.  osp_result_info(out) is in's with nnz_c and ms_total replaced (M, N and
 * dtype are in's).
 *
 * A null in, sel or out, an op outside osp_select_op_t, a non-zero reserved word and a result of osp_spgemm_partials are
 * OSP_ERR_ARG.  On any error *out and *stats are left as they were.  An empty `in` and M == 0 are legal and launch no select
 * kernel.
 *
 * Cost: a value predicate reads in's values once (and nothing else) for the verdicts, a position predicate in's columns and
 * the row pointers its chunks span; then the kept entries are read once more and written.  One read-back per call (nnz_out).
 * Everything runs on the context's stream with temporary buffers from its pool; the work is cut by entries of `in`, so a few
 * very long rows cost what many short ones cost.
 *
 * stats (may be NULL): nnz_in / nnz_out, ms_total = device time of the call, launches = kernels launched (copies not
 * counted), reserved = 0.
 */
int osp_csr_select(osp_result_t in, const osp_select_t *sel, osp_result_t *out, osp_select_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_SELECT_H */
