/*
 * outerspace_spgemm_scan.h -- the row-wise inclusive scan of a CSR result and weighted draws from its rows on an AMD
 * Instinct MI355X (gfx950): a running sum, minimum or maximum along every row of a CSR result that already exists, and s
 * draws per row, with replacement, in proportion to the row's values -- without leaving the device.
 *
 * Every other operation on a result decides an entry on its own (select, apply_mask, apply_vectors, ...) or folds a whole
 * row to one value (reduce, mxv, ...).  This header adds the third kind: a value per entry that depends on the entries
 * before it in its row.  Its first client is inverse-CDF sampling: a per-row CDF and one bisection per draw.  Two functions,
 * no change to any existing struct (OSP_VERSION stays as outerspace_spgemm.h, which this header includes, gives it).  No
 * reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_SCAN_H
#define OUTERSPACE_SPGEMM_SCAN_H

#include "outerspace_spgemm_vector.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSP_SCAN_BLOCK 32   /* kScanBlock: entries of one block of the scan order below */

typedef struct osp_scan {
    int32_t  op;            /* OSP_REDUCE_PLUS, OSP_REDUCE_MIN or OSP_REDUCE_MAX (osp_reduce_op_t) */
    uint32_t reserved[8];   /* must be 0 */
} osp_scan_t;

typedef struct osp_scan_stats {
    uint64_t nnz_in;        /* entries of `in` */
    uint64_t nnz_out;       /* entries of `out`: nnz_in */
    uint64_t blocks;        /* nnz_in / 32 + M: the blocks the kernels are launched for.  The exact number, the sum of
                               ceil(m_i / 32) over the rows, is at most this and stays on the device */
    float    ms_total;      /* device time of the call */
    uint32_t launches;      /* kernels launched (copies and memsets not counted) */
    uint32_t readbacks;     /* values read back by the host: 0 */
    uint32_t reserved[7];   /* written 0 */
} osp_scan_stats_t;

/*
 * out = the inclusive scan of every row of `in` under sc->op.
 *   in    -- any CSR result (not one of osp_spgemm_partials); it stays valid
 *   sc    -- the operator
 *
 * out has in's pattern (row pointers and columns are copied); osp_result_info(out) is in's with ms_total replaced.  The
 * value at the q-th entry of a row of m entries e_0 .. e_{m-1} (ascending columns) is S_q:
 *
 *   id and a (+) b are osp_csr_reduce's: PLUS: id = +0.0, a (+) b = ONE IEEE addition, never contracted;
 *                                        MIN:  id = +inf, a (+) b = b < a ? b : a;
 *                                        MAX:  id = -inf, a (+) b = b > a ? b : a.
 *   The row is cut into consecutive blocks of OSP_SCAN_BLOCK = 32 entries; the last block may be shorter.
 *   Inside block b, sequentially:           L_first = id (+) e_first,   L_q = L_{q-1} (+) e_q;
 *                                           T_b = the L of the block's last entry.
 *   Across the blocks of the row, sequentially:   C_0 = id,   C_{b+1} = C_b (+) T_b.
 *   S_q = C_b (+) L_q   for q in block b.
 *
 * What follows from it:
 *   - a row of at most 32 entries is the sequential running sum (numpy.cumsum in the dtype, for PLUS) except that a leading
 *     -0.0 reads +0.0, as in osp_csr_reduce; in block 0, S_q has L_q's bits;
 *   - MIN and MAX never return a NaN: a NaN entry is never taken, and id is returned until a number arrives;
 *   - PLUS propagates a NaN from its position to the end of the row (which NaN -- its sign and payload -- is not specified);
 *   - a row's scan depends on the row's values alone, not on where the row lies or on any other row;
 *   - for PLUS on entries that are all >= 0 and not NaN, S is non-decreasing, and an entry equal to 0 beyond the row's
 *     first has S_q == S_{q-1} bit for bit.  (Inside a block fl(C + L) is monotone in L; across a boundary the block's last
 *     S is fl(C_b + T_b) = C_{b+1} and the next block's first is fl(C_{b+1} + x) >= C_{b+1}.  A scan by doubling inside
 *     a wave, or more than two levels, loses this by an ulp.)
 *
 * A null in, sc or out, an op outside the three (COUNT included), a non-zero reserved word and a result of
 * osp_spgemm_partials are OSP_ERR_ARG.  On any error *out and *stats are left as they were.  An empty `in` and M == 0 are
 * legal and launch no kernel.
 *
 * Cost: the block count of every row is scanned into a block table; a lane per block runs the 32 sequential steps on
 * entries staged through LDS; the rows of more than one block get their C_b from one lane (up to 16 blocks) or one wave, and
 * one more pass over the entries adds C_b in place.  The last two are not launched when min(N, nnz) <= 32: no row then has
 * a second block.  Nothing is read back.
 *
 * stats (may be NULL): as the struct says.
 */
int osp_csr_scan(osp_result_t in, const osp_scan_t *sc, osp_result_t *out, osp_scan_stats_t *stats /* may be NULL */);

typedef struct osp_draw {
    uint32_t draws;         /* s >= 1: draws per row */
    uint32_t reserved0;     /* must be 0 */
    uint64_t seed;
    uint32_t reserved[8];   /* must be 0 */
} osp_draw_t;

typedef struct osp_draw_stats {
    uint64_t nnz_in;        /* entries of `in` */
    uint64_t nnz_out;       /* M * s: values written to cols (and to pos) */
    uint64_t rows_without;  /* rows that cannot be drawn from: their draws are -1 */
    float    ms_total;      /* device time of the call */
    uint32_t launches;      /* kernels launched (copies and memsets not counted) */
    uint32_t readbacks;     /* values read back by the host: 1 (rows_without) */
    uint32_t reserved[7];   /* written 0 */
} osp_draw_stats_t;

/*
 * dr->draws = s weighted draws from every row of `in`, with replacement: row-major, cols[i s + d] is the column of the
 * entry that draw d of row i picked and pos[i s + d] that entry's index in in's arrays (osp_result_csr); both are -1 where
 * the row cannot be drawn from.
 *   in    -- any CSR result (not one of osp_spgemm_partials); it stays valid
 *   cols  -- M * s int64 values in `space`; pos -- the same, or NULL
 *
 * Weights:   w_q = (e_q > 0 && e_q < +inf) ? e_q : +0.0.  Zeros, negatives, NaNs and infinities are never drawn and never
 *            poison the row.
 * CDF:       S = osp_csr_scan's PLUS scan of w, to the bit.
 * Drawable:  total = S_{m-1}; a row is drawable when 0 < total < +inf.  Every other row -- an empty one, one without a
 *            positive finite weight, one whose sum overflows -- gives -1 and counts in stats.rows_without.
 * Number:    h = mix(s0 ^ ((uint64)i << 32 | d)),  s0 = mix(seed + 0x9E3779B97F4A7C15),  mix as in
 *            outerspace_spgemm_select_k.h (the draw number in the column's place);
 *            f64: u = (h >> 11) * 2^-53;  f32: u = (h >> 40) * 2^-24  (both exact, in [0, 1));
 *            t = u * total, one IEEE multiplication in the dtype.
 * Pick:      the first q with S_q > t || S_q == total.  S is non-decreasing, so this is one bisection; the second clause
 *            only matters when u * total rounds up to total.  An entry of weight 0 is never the first to satisfy the
 *            predicate (beyond the row's first its S equals the one before; at the row's first S_0 = 0 is neither > t nor
 *            == total).
 * For a fixed seed, a row's draws depend on the row's number and values alone.
 *
 * A null in, dr or cols, draws == 0, M * draws > 2^40, a non-zero reserved word, a space outside osp_memspace_t and a result
 * of osp_spgemm_partials are OSP_ERR_ARG.  On any error cols, pos and *stats are left as they were.  An empty `in` and
 * M == 0 are legal and launch no kernel (every draw of an empty `in` is -1).
 *
 * Cost: the scan above into a temporary of nnz values, then a lane per (row, draw): two row pointers, the total, the hash
 * and a bisection of the row's slice of S.  cols (and pos, only when it is given) are formed in temporaries of M * s values
 * and copied out last.  Nothing is read back unless stats is given: rows_without then costs one more small kernel and ONE
 * read-back.
 */
int osp_csr_draw(osp_result_t in, const osp_draw_t *dr, int64_t *cols /* M x s */, int64_t *pos /* M x s, may be NULL */,
                 osp_memspace_t space, osp_draw_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_SCAN_H */
