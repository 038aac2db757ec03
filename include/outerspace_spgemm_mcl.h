/*
 * outerspace_spgemm_mcl.h -- the step between two expansions of Markov clustering (MCL) on an AMD Instinct MI355X
 * (gfx950): prune, inflate and normalise the rows of a CSR result without leaving the device.
 *
 * MCL repeats  expand (T <- T*T) -> prune -> inflate -> normalise  until the walk matrix T stops changing.  Expansion is a
 * product of outerspace_spgemm.h (which this header includes); this header adds everything between two products.  T is
 * kept ROW-stochastic (the transpose of the textbook's column-stochastic matrix), so every step works on CSR rows.
 * No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_MCL_H
#define OUTERSPACE_SPGEMM_MCL_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osp_mcl_step {          /* zero-initialise; reserved must be 0 */
    double   power;         /* inflation exponent r >= 1.  1: values kept as they are; 2: v*v; else pow(v, r) */
    double   threshold;     /* prune: an entry survives iff v >= threshold (0: keep all) */
    uint32_t max_per_row;   /* then keep at most this many entries of a row, the largest ones (0: no cap) */
    uint32_t reserved[5];
} osp_mcl_step_t;

typedef struct osp_mcl_stats {
    uint64_t nnz_in, nnz_out;
    uint64_t rows_capped;      /* rows that lost entries to max_per_row */
    uint64_t rows_rescued;     /* non-empty rows with nothing >= threshold: their largest entry was kept */
    uint64_t rows_long;        /* rows handled by the long-row (one workgroup per row) path */
    double   chaos;            /* max over rows of  max_j out[i,j] - sum_j out[i,j]^2 ; 0 for a converged matrix */
    float    ms_total, ms_select_kernel;
    uint32_t launches;
    uint32_t reserved[5];
} osp_mcl_stats_t;

/*
 * out = normalise(inflate(prune(in))), row by row.  `in` is any CSR result (not one of osp_spgemm_partials) and stays
 * valid; `out` is an ordinary osp_result_t on the same context with exact row pointers and ascending columns, taken by
 * every osp_result_* function, osp_csr_bias_relu and osp_csr_inflate_prune.  osp_result_info(out) is in's with nnz_c and
 * ms_total replaced (M, N and dtype are in's).
 *
 * Per row, with threshold and power converted to the value type first (float for OSP_F32):
 *   1. Prune.  Keep the entries with v >= threshold.  If a non-empty row keeps nothing, keep its single largest entry
 *      (rows_rescued).  If more than max_per_row remain, keep the max_per_row largest (rows_capped).  Among equal values
 *      the lower column wins.  The kept entries stay in ascending column order.  An empty row stays empty.
 *      (-0.0 orders as +0.0.)
 *   2. Inflate.  w = v for power == 1, w = v*v for power == 2 (one rounding), otherwise w = pow(v, power).
 *   3. Normalise.  out = w / s (IEEE division), s the sum of the row's w.  A row whose kept w are all zero divides 0 by 0.
 *   4. Chaos.  max(out) - sum(out*out) of the row, in the value type; stats->chaos is the largest over all rows, a row
 *      whose difference rounds below zero and an empty row counting as 0.
 *
 * Order of additions (results are defined to the bit).  Both sums, s and sum(out*out), run over the row's kept entries
 * e_0 .. e_{m-1} in ascending column order:  p_l = e_l + e_{l+64} + e_{l+128} + ...  left to right for l = 0..63 (a
 * missing p_l is +0.0), then  for d in 32, 16, 8, 4, 2, 1:  p_l += p_{l+d} for l < d;  the sum is p_0.  No product is
 * contracted into an addition.  The order depends on the row's kept values and their count alone.
 *
 * Values must be finite and >= 0.  With validate != 0 a negative, NaN or infinite value is OSP_ERR_ARG, checked on the
 * device before anything is written; without it the result for such input is unspecified (no access leaves the arrays).
 * power < 1 or NaN, a NaN or negative threshold, a non-zero reserved word, a null in, step or out, or a result of
 * osp_spgemm_partials is OSP_ERR_ARG.  On any error *out and *stats are left as they were.  An `in` without entries, M == 0
 * and N == 0 included, is legal: out is an empty M x N result and every row counter is 0.
 *
 * stats (may be NULL): nnz_in / nnz_out, the row counters above, rows_long = the rows longer than the library's class
 * boundary (one workgroup each instead of one wave), ms_total = device time of the call, ms_select_kernel = the part of
 * it spent in the kernels that select, compact and normalise, launches = kernels launched.
 */
int osp_csr_inflate_prune(osp_result_t in, const osp_mcl_step_t *step, int validate,
                          osp_result_t *out, osp_mcl_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_MCL_H */
