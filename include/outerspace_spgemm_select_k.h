/*
 * outerspace_spgemm_select_k.h -- the row-wise k-select of a CSR result on an AMD Instinct MI355X (gfx950): keep, of every
 * row of a CSR result that already exists, the k entries that rank first under an order -- the largest values, the smallest
 * values, or a uniform random choice -- without leaving the device.
 *
 * osp_csr_select (outerspace_spgemm_select.h) and osp_csr_apply_mask decide an entry on its own; this header decides it by
 * its rank inside its row.  It is the step of neighbour sampling between two extracts ("at most fanout random neighbours of
 * each frontier vertex"), of a k-nearest-neighbour sparsification after a similarity product, and of one step of a uniform
 * random walk.  It adds ONE function and changes no existing struct (OSP_VERSION stays as outerspace_spgemm.h, which this
 * header includes, gives it).  No reference counterpart.
 */
#ifndef OUTERSPACE_SPGEMM_SELECT_K_H
#define OUTERSPACE_SPGEMM_SELECT_K_H

#include "outerspace_spgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OSP_SELECT_K_LARGEST = 0,    /* the k largest values */
    OSP_SELECT_K_SMALLEST = 1,   /* the k smallest values */
    OSP_SELECT_K_RANDOM = 2      /* k entries chosen by a hash of (seed, row, column) */
} osp_select_k_order_t;

typedef struct osp_select_k {
    int32_t  order;         /* osp_select_k_order_t */
    uint32_t k;             /* >= 1: a row keeps min(its length, k) entries */
    uint64_t seed;          /* RANDOM only; ignored otherwise */
    uint32_t reserved[8];   /* must be 0 */
} osp_select_k_t;

typedef struct osp_select_k_stats {
    uint64_t nnz_in;        /* entries of `in` */
    uint64_t nnz_out;       /* entries of `out` */
    uint64_t rows_capped;   /* rows longer than k */
    uint64_t rows_long;     /* capped rows selected by a whole workgroup instead of one wave */
    float    ms_total;      /* device time of the call */
    uint32_t launches;      /* kernels launched (copies and memsets not counted) */
    uint32_t readbacks;     /* values read back by the host */
    uint32_t reserved[6];   /* written 0 */
} osp_select_k_stats_t;

/*
 * out = of every row of `in`, the sk->k entries that come first under sk->order.
 *   in    -- any CSR result (not one of osp_spgemm_partials); it stays valid
 *   sk    -- the order, k and the seed
 *
 * A row of m entries keeps all of them when m <= k; otherwise it keeps the k entries that come first under the order below
 * (the row is then not read past the select).  Kept entries keep their value bits (NaN payloads and -0.0 included: values are
 * copied, never computed), columns stay ascending, row pointers are exact -- out.rowptr[i + 1] - out.rowptr[i] ==
 * min(m_i, k) -- and out is allocated at its exact size.  The select is structural: an explicit zero is an entry like any
 * other.  out is an ordinary osp_result_t on in's context, taken by every function that takes a result;
 * osp_result_info(out) is in's with nnz_c and ms_total replaced.
 *
 * LARGEST:  a comes before b when a > b under IEEE comparison: -0.0 equals +0.0; every number, +-inf included, comes before
 *           every NaN; all NaNs are equal to one another.  Among equals the lower column comes first.  (This is
 *           osp_csr_inflate_prune's tie rule: on finite non-negative input LARGEST keeps the pattern that
 *           inflate_prune(power 1, threshold 0, max_per_row k) keeps.)
 * SMALLEST: the same with a < b.  NaNs are still last.
 * RANDOM:   values are never read by the select.  The entry at (row i, column j) has the 64-bit key
 *               mix(s ^ ((uint64)i << 32 | j))    with    s = mix(seed + 0x9E3779B97F4A7C15),
 *               mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
 *           (all arithmetic mod 2^64), and the smaller key comes first.  For a fixed seed the key is a bijection of (i, j)
 *           -- M and N are below 2^32 -- so there are no ties and no tie rule.  The selection of a row depends on the seed,
 *           the row's number and its set of columns alone: not on values, dtype, the other rows or any launch geometry.
 *           Over seeds, every k-subset of a row is (to the quality of the hash) equally likely.
 *
 * For all three orders: select with k, then select with k' <= k under the same order and seed, equals the select with k'
 * alone; and a k that no row exceeds returns `in` bit for bit and launches no select kernel.
 *
 * A null in, sk or out, an order outside osp_select_k_order_t, k == 0, a non-zero reserved word and a result of
 * osp_spgemm_partials are OSP_ERR_ARG.  On any error *out and *stats are left as they were.  An empty `in` and M == 0 are
 * legal and launch no kernel.
 *
 * Cost: one pass over the row pointers lists the rows longer than k; each of those is read at most (bytes of the key) + 1
 * times by one wave -- by one workgroup of 256 when it is longer than 2048 entries -- to find its threshold (a radix select,
 * 8 bits a pass, that stops as soon as a bucket is taken whole; keys are 4 bytes for an f32 value order, 8 for f64 and
 * RANDOM); then every entry is flagged once (a value order reads its value, RANDOM its column), and the kept entries are read
 * once more and written.  Two read-backs per call (the classes' sizes, nnz_out); one when no row is capped; none when
 * k >= min(N, nnz), which the host sees without asking.  Everything runs on the context's stream with temporary buffers from
 * its pool.
 *
 * stats (may be NULL): nnz_in / nnz_out, rows_capped / rows_long, ms_total = device time of the call, launches = kernels
 * launched, readbacks, reserved = 0.
 */
int osp_csr_select_k(osp_result_t in, const osp_select_k_t *sk, osp_result_t *out, osp_select_k_stats_t *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* OUTERSPACE_SPGEMM_SELECT_K_H */
