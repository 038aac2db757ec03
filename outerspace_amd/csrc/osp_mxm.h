// osp_mxm.h -- the row-wise (Gustavson) product of two CSR results under a named semiring (osp_csr_mxm,
// include/outerspace_spgemm_mxm.h), written for gfx950 (wave64).  DESIGN.md section 15.
//
// Both operands are results: CSR, columns ascending.  Row i of the output is the fold of the rows B[k,:] over the entries
// A[i,k], so walking A's row and B's rows yields the row's products in (k ascending, column ascending) order, and a STABLE
// sort by column leaves the products of one output entry in ascending k: the order the fold is defined in.
//
//   symbolic   w[p] = nnz(B[k,:]) for entry p of a (k its column); wscan = the exclusive scan of w.  The products of row i
//              are wscan[a.rowptr[i]] .. wscan[a.rowptr[i + 1]]: ONE array gives a row's product count U_i, its place in the
//              expansion, and (by a bisection between the row's ends) the entry of a that owns a product.
//   batches    consecutive rows of at most `budget` products (mxm_cut_kernel); everything below is per batch, and every
//              temporary is sized by the batch.
//   short rows U_i <= cap: one wave per row (mxm_short_kernel).  Products go straight into LDS as (column << 32 | t, value),
//              t the product's position; the keys are unique, so a bitonic sort of them IS a stable sort by column; runs of
//              equal columns are folded by a lane each, left to right, and the compressed row goes to the row's slot.  A
//              short row's products never touch HBM.
//   long rows  U_i > cap: listed, expanded by products (mxm_expand_kernel, a lane per product whatever the row), sorted by
//              (long-row rank, column) with the library's stable radix sort (ONE sort for all long rows of the batch: the
//              launch count does not depend on their number), heads of equal keys flagged and scanned, and every run folded
//              in sorted order (mxm_fold_kernel: a run of more than 64 by its wave, 64 values per coalesced load, combined one
//              after another as heavy_reduce_kernel does).
//   output     a row's slot is its place in the expansion (it holds at most U_i entries); the per-row counts are scanned,
//              ONE read-back sizes the batch's output, and mxm_gather_kernel moves the slots' entries there, cut by entries.
//
// mul is applied where products are formed, add where they are folded: the two never meet in one instantiation's inner
// loop.  The expansion is instantiated per mul, the folds per add; the short kernel is instantiated per add and selects its
// product loop by a wave-uniform switch on mul.  Values that are only moved are moved as integers of their width.
// No float atomics, no waiting between workgroups, no scratch.
//
// The MASKED form (osp_csr_mxm_masked, include/outerspace_spgemm_mxm_masked.h) drops a product whose
// (row, column) a CSR pattern rejects where the product is formed.  The short kernel and the expansion are templated on it
// (`if constexpr`: the unmasked instantiations run the instructions they ran; each takes one more by-value argument it never
// reads, so the kernarg layout grew); everything after the expansion is the same code working on the kept products only.
//   short rows the products are formed in rounds of 64 in (k, column) order; a lane bisects its product's column in mask row
//              i (read by this one wave: it stays in cache), and the survivors go to LDS compacted in the same order (ballot,
//              prefix popcount).  The key is (column << 32 | compact position): unique, so the sort stays stable by column,
//              and its padded length follows the KEPT count.  A rejected product's values are not loaded.
//   long rows  mxm_mask_flag_kernel (a lane per formed product, no value read) writes one verdict bit per product; the scan
//              of the words' popcounts (osp_compact.h) and mxm_kept_list_kernel give the kept products' original positions
//              and the long rows' KEPT offsets; the expansion takes a lane per kept product, and the sort, the fold and the
//              counts see the kept offsets.  Positions stay 32 bits.
#pragma once
#include "osp_compact.h"
#include "osp_ewise.h"

namespace osp {

constexpr uint32_t kMxmShortMax = 1024;              // a short row's products: 16 KiB of LDS per wave at f64 (10 waves a CU)
constexpr uint64_t kMxmBatchDefault = 1ull << 24;    // products per batch
enum { MXM_NSHORT = 0, MXM_NLONG, MXM_NTOOBIG, MXM_COUNTERS };

// ---- symbolic -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mxm_entry_len_kernel(const uint32_t *__restrict__ a_col, uint64_t nnz_a, const int64_t *__restrict__ b_rowptr,
                                                            uint32_t *__restrict__ w) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_a) return;
    const uint32_t k = a_col[p];
    w[p] = (uint32_t)(b_rowptr[k + 1] - b_rowptr[k]);
}
// rows by class, and the rows whose positions would not fit 32 bits
__global__ __launch_bounds__(256) void mxm_classify_kernel(const int64_t *__restrict__ a_rowptr, uint64_t M, const uint64_t *__restrict__ wscan,
                                                           uint32_t cap, unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t u = 0;
    if (i < M) u = wscan[a_rowptr[i + 1]] - wscan[a_rowptr[i]];
    const uint64_t sh = __ballot(u > 0 && u <= cap), lg = __ballot(u > cap), big = __ballot(u >= 0xffffffffull);
    if (lane_id() == 0) {
        if (sh) atomicAdd(&counters[MXM_NSHORT], (unsigned long long)__popcll(sh));
        if (lg) atomicAdd(&counters[MXM_NLONG], (unsigned long long)__popcll(lg));
        if (big) atomicAdd(&counters[MXM_NTOOBIG], (unsigned long long)__popcll(big));
    }
}
// The batches, by one thread: a batch begins at row r and takes the rows after it while the products stay within `budget`
// (at least one row).  cuts[2 t] is batch t's first row, cuts[2 t + 1] the products before it; a last pair (M, products)
// closes the list.  *nb = the number of batches, or max_batches + 1 when the list is too short (never, by its bound).
__global__ void mxm_cut_kernel(const int64_t *__restrict__ a_rowptr, const uint64_t *__restrict__ wscan, uint64_t M, uint64_t budget,
                               uint32_t max_batches, uint64_t *__restrict__ cuts, uint32_t *__restrict__ nb) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t r = 0;
    uint32_t t = 0;
    while (r < M) {
        if (t == max_batches) { *nb = max_batches + 1; return; }
        const uint64_t off = wscan[a_rowptr[r]], target = off + budget;
        cuts[2 * t] = r;
        cuts[2 * t + 1] = off;
        t++;
        uint64_t lo = r + 1, hi = M + 1;   // the first row index in (r, M] whose products begin beyond the target, or M + 1
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (wscan[a_rowptr[mid]] <= target) lo = mid + 1; else hi = mid;
        }
        r = lo - 1 > r ? lo - 1 : r + 1;
    }
    cuts[2 * t] = M;
    cuts[2 * t + 1] = wscan[a_rowptr[M]];
    *nb = t;
}

// mul(a, b) with the operator a wave-uniform run-time value (the short kernel's product loop)
template <class T, class V>
__device__ __forceinline__ V mxm_mul(int mul, V a, V b) {
    switch (mul) {
        case EW_PLUS: return ewise_apply<EW_PLUS, T, V>(a, b);
        case EW_TIMES: return ewise_apply<EW_TIMES, T, V>(a, b);
        case EW_MIN: return ewise_apply<EW_MIN, T, V>(a, b);
        case EW_MAX: return ewise_apply<EW_MAX, T, V>(a, b);
        case EW_FIRST: return a;
        default: return b;   // EW_SECOND
    }
}

// the entry of a that owns product t of the row whose entries are [e0, e1) and whose products begin at w0: the last e with
// wscan[e] <= w0 + t (an entry that meets an empty row of b owns no product and is never the last such e)
__device__ __forceinline__ uint64_t mxm_owner(const uint64_t *__restrict__ wscan, uint64_t e0, uint64_t e1, uint64_t x) {
    return upper_bound_dev(wscan, e0, e1, x) - 1;
}

// The mask of the masked form, as the kernels take it: a CSR pattern with the output's shape, the sense, and the call's count
// of kept products of short rows.  The unmasked instantiations never touch it.
struct MxmMask {
    const int64_t *rowptr;
    const uint32_t *col;
    int complement;
    unsigned long long *kept_short;
};
// the verdict on a product at column j of output row i: the mask holds (i, j), or -- complemented -- does not
__device__ __forceinline__ bool mxm_mask_admits(const MxmMask &m, uint64_t i, uint32_t j) {
    const uint64_t m1 = (uint64_t)m.rowptr[i + 1];
    const uint64_t at = lower_bound_dev(m.col, (uint64_t)m.rowptr[i], m1, j);
    const bool member = at < m1 && m.col[at] == j;
    return member != (m.complement != 0);
}

// ---- short rows: one wave per row of the batch ------------------------------------------------------------------------------
// grid: the batch's rows; block: one wave.  A row without products gets its count 0 here, a long row is left to the long path.
// MASKED: only the products the mask admits enter LDS, compacted in their order; U below is then the KEPT count (a row that
// keeps nothing gets its count 0), and the slot is still the row's place among the FORMED products.
template <class T, int ADD, bool MASKED>
__global__ __launch_bounds__(kWave) void mxm_short_kernel(const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col,
                                                          const ValueBits<T> *__restrict__ a_val, const int64_t *__restrict__ b_rowptr,
                                                          const uint32_t *__restrict__ b_col, const ValueBits<T> *__restrict__ b_val,
                                                          const uint64_t *__restrict__ wscan, uint64_t r0, uint32_t cap, int mul, uint64_t p0,
                                                          uint32_t *__restrict__ tcol, ValueBits<T> *__restrict__ tval, uint32_t *__restrict__ cnt,
                                                          MxmMask mask) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    __shared__ uint64_t skey[kMxmShortMax];
    __shared__ V sval[kMxmShortMax];
    const uint64_t i = r0 + blockIdx.x;
    const uint64_t e0 = (uint64_t)a_rowptr[i], e1 = (uint64_t)a_rowptr[i + 1];
    const uint64_t w0 = wscan[e0], u64 = wscan[e1] - w0;
    const unsigned lane = threadIdx.x;
    if (u64 == 0) {
        if (lane == 0) cnt[i] = 0;
        return;
    }
    if (u64 > cap) return;
    uint32_t U = (uint32_t)u64;
    uint32_t n2 = 1;   // the sorted length: a power of two, padded with keys above every real one
    if constexpr (!MASKED) {
        while (n2 < U) n2 <<= 1;
        // 1. the products, in (k ascending, column ascending) order
        for (uint32_t t = lane; t < n2; t += kWave) {
            uint64_t key = ~0ull;
            if (t < U) {
                const uint64_t e = mxm_owner(wscan, e0, e1, w0 + t);
                const uint64_t q = (uint64_t)b_rowptr[a_col[e]] + (w0 + t - wscan[e]);
                key = ((uint64_t)b_col[q] << 32) | t;
                sval[t] = mxm_mul<T, V>(mul, a_val[e], b_val[q]);
            }
            skey[t] = key;
        }
    } else {
        // 1. the products the mask admits, in (k ascending, column ascending) order: rounds of 64 formed products, the
        // survivors of a round behind those of the rounds before it (a compact position never exceeds the formed one)
        uint32_t kept = 0;
        for (uint32_t base = 0; base < U; base += kWave) {
            const uint32_t t = base + lane;
            bool keep = false;
            uint64_t e = 0, q = 0;
            uint32_t col = 0;
            if (t < U) {
                e = mxm_owner(wscan, e0, e1, w0 + t);
                q = (uint64_t)b_rowptr[a_col[e]] + (w0 + t - wscan[e]);
                col = b_col[q];
                keep = mxm_mask_admits(mask, i, col);
            }
            const uint64_t keeps = __ballot(keep);
            if (keep) {
                const uint32_t c = kept + (uint32_t)__popcll(keeps & lanemask_lt());
                skey[c] = ((uint64_t)col << 32) | c;
                sval[c] = mxm_mul<T, V>(mul, a_val[e], b_val[q]);
            }
            kept += (uint32_t)__popcll(keeps);
        }
        U = kept;
        if (U == 0) {
            if (lane == 0) cnt[i] = 0;
            return;
        }
        if (lane == 0) atomicAdd(mask.kept_short, (unsigned long long)U);
        while (n2 < U) n2 <<= 1;
        for (uint32_t t = U + lane; t < n2; t += kWave) skey[t] = ~0ull;
    }
    __syncthreads();
    // 2. bitonic sort of the unique keys (column, position): stable by column
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < n2; t += kWave) {
                const uint32_t x = t ^ j;
                if (x > t) {
                    const uint64_t a = skey[t], b = skey[x];
                    if ((a > b) == ((t & k) == 0)) {
                        skey[t] = b;
                        skey[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // 3. a lane per run of equal columns, folded left to right from the first product; 4. the compressed row
    const uint64_t slot = w0 - p0;
    uint32_t nheads = 0;
    for (uint32_t base = 0; base < U; base += kWave) {
        const uint32_t t = base + lane;
        const bool valid = t < U;
        const uint64_t key = valid ? skey[t] : 0ull;
        const uint32_t col = (uint32_t)(key >> 32);
        const bool head = valid && (t == 0 || (uint32_t)(skey[t - 1] >> 32) != col);
        const uint64_t heads = __ballot(head);
        if (head) {
            V acc = sval[(uint32_t)key];
            for (uint32_t v = t + 1; v < U; v++) {
                const uint64_t kv = skey[v];
                if ((uint32_t)(kv >> 32) != col) break;
                acc = ewise_apply<ADD, T, V>(acc, sval[(uint32_t)kv]);
            }
            const uint64_t o = slot + nheads + (uint32_t)__popcll(heads & lanemask_lt());
            tcol[o] = col;
            tval[o] = acc;
        }
        nheads += (uint32_t)__popcll(heads);
    }
    if (lane == 0) cnt[i] = nheads;
}

// ---- long rows ----------------------------------------------------------------------------------------------------------------
// per row x of the batch: flag[x] = the row is long, lp[x] = its products when it is
__global__ __launch_bounds__(256) void mxm_long_flag_kernel(const int64_t *__restrict__ a_rowptr, const uint64_t *__restrict__ wscan, uint64_t r0,
                                                            uint64_t nrows, uint32_t cap, uint32_t *__restrict__ flag, uint32_t *__restrict__ lp) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nrows) return;
    const uint64_t u = wscan[a_rowptr[r0 + x + 1]] - wscan[a_rowptr[r0 + x]];
    flag[x] = u > cap ? 1u : 0u;
    lp[x] = u > cap ? (uint32_t)u : 0u;
}
// the long rows in row order and the first product of each in the batch's expansion; loff[number of long rows] = their products
__global__ __launch_bounds__(256) void mxm_long_list_kernel(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank,
                                                            const uint64_t *__restrict__ lpscan, uint64_t r0, uint64_t nrows,
                                                            uint32_t *__restrict__ long_rows, uint64_t *__restrict__ loff) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > nrows) return;
    if (x == nrows) { loff[rank[nrows]] = lpscan[nrows]; return; }
    if (flag[x]) {
        long_rows[rank[x]] = (uint32_t)(r0 + x);
        loff[rank[x]] = lpscan[x];
    }
}
// a lane per product of the long rows: key = (long-row rank << colbits) | column, payload = the product's position.
// MASKED: a lane per KEPT product x; kept_pos[x] is its position among the FORMED products of the long rows, which loff (the
// formed offsets) decodes; keys, positions and values are written at x, so what follows sees the kept products only.
template <class T, int MUL, bool MASKED>
__global__ __launch_bounds__(256) void mxm_expand_kernel(const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col,
                                                         const ValueBits<T> *__restrict__ a_val, const int64_t *__restrict__ b_rowptr,
                                                         const uint32_t *__restrict__ b_col, const ValueBits<T> *__restrict__ b_val,
                                                         const uint64_t *__restrict__ wscan, const uint32_t *__restrict__ long_rows,
                                                         const uint64_t *__restrict__ loff, uint32_t nlong, uint64_t nprod, int colbits,
                                                         uint64_t *__restrict__ key, uint32_t *__restrict__ pos, ValueBits<T> *__restrict__ pval,
                                                         const uint32_t *__restrict__ kept_pos) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nprod) return;
    uint64_t y = x;   // the product's position among the formed products of the long rows
    if constexpr (MASKED) y = kept_pos[x];
    const uint64_t h = upper_bound_dev(loff, 0, (uint64_t)nlong + 1, y) - 1;
    const uint64_t i = long_rows[h];
    const uint64_t e0 = (uint64_t)a_rowptr[i], e1 = (uint64_t)a_rowptr[i + 1];
    const uint64_t w = wscan[e0] + (y - loff[h]);
    const uint64_t e = mxm_owner(wscan, e0, e1, w);
    const uint64_t q = (uint64_t)b_rowptr[a_col[e]] + (w - wscan[e]);
    key[x] = (h << colbits) | (uint64_t)b_col[q];
    pos[x] = (uint32_t)x;
    // (FIRST reads no value of b, SECOND none of a: the unused load is gone with the constant MUL)
    pval[x] = ewise_apply<MUL, T, V>(MUL == EW_SECOND ? (V)0 : a_val[e], MUL == EW_FIRST ? (V)0 : b_val[q]);
}
// ---- the masked form's long rows: one verdict bit per formed product, then the kept products listed ------------------------------
// a lane per formed product x of the batch's long rows (decoded as the expansion decodes it): the owner, the column, a
// bisection in the mask row, a verdict.  No value is read.  The 64 verdicts of a wave are word x >> 6 of `bits`.
__global__ __launch_bounds__(256) void mxm_mask_flag_kernel(const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col,
                                                            const int64_t *__restrict__ b_rowptr, const uint32_t *__restrict__ b_col,
                                                            const uint64_t *__restrict__ wscan, const uint32_t *__restrict__ long_rows,
                                                            const uint64_t *__restrict__ loff, uint32_t nlong, uint64_t nprod, MxmMask mask,
                                                            uint64_t *__restrict__ bits) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (x < nprod) {
        const uint64_t h = upper_bound_dev(loff, 0, (uint64_t)nlong + 1, x) - 1;
        const uint64_t i = long_rows[h];
        const uint64_t e0 = (uint64_t)a_rowptr[i], e1 = (uint64_t)a_rowptr[i + 1];
        const uint64_t w = wscan[e0] + (x - loff[h]);
        const uint64_t e = mxm_owner(wscan, e0, e1, w);
        const uint64_t q = (uint64_t)b_rowptr[a_col[e]] + (w - wscan[e]);
        keep = mxm_mask_admits(mask, i, b_col[q]);
    }
    store_verdicts(keep, x, nprod, bits);
}
// kpos: the exclusive scan of the words' popcounts.  kept_pos[c] = the formed position of the c-th kept product (a lane per
// formed product), and kloff[h] = the kept products before long row h, kloff[nlong] = all of them (a lane per long row, the
// expression of compact_rowptr_kernel).
__global__ __launch_bounds__(256) void mxm_kept_list_kernel(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ kpos, uint64_t nprod,
                                                            const uint64_t *__restrict__ loff, uint32_t nlong, uint32_t *__restrict__ kept_pos,
                                                            uint64_t *__restrict__ kloff) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nprod) {
        const uint64_t word = bits[x >> 6];
        if ((word >> (x & 63)) & 1ull) kept_pos[kpos[x >> 6] + (uint64_t)__popcll(word & ((1ull << (x & 63)) - 1ull))] = (uint32_t)x;
    }
    if (x <= nlong) {
        const uint64_t p = loff[x];
        uint64_t o = kpos[p >> 6];
        if (p & 63) o += (uint64_t)__popcll(bits[p >> 6] & ((1ull << (p & 63)) - 1ull));   // (p & 63 == 0: the word may not exist)
        kloff[x] = o;
    }
}
// the long rows of a batch in which no long row keeps a product: nothing is sorted, every count is 0
__global__ __launch_bounds__(256) void mxm_long_empty_kernel(const uint32_t *__restrict__ long_rows, uint32_t nlong, uint32_t *__restrict__ cnt) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < nlong) cnt[long_rows[h]] = 0;
}

template <class V>
__global__ __launch_bounds__(256) void mxm_sorted_values_kernel(const uint32_t *__restrict__ pos, const V *__restrict__ pval, uint64_t n,
                                                                V *__restrict__ sorted_val) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) sorted_val[x] = pval[pos[x]];
}
// One thread per run of equal (long row, column) keys: folded in sorted order (= ascending position = ascending k) from its
// first value, and written to the row's slot.  A run of more than 64 values is folded by the whole wave in the same order.
template <class T, int ADD>
__global__ __launch_bounds__(256) void mxm_fold_kernel(const uint64_t *__restrict__ key, const ValueBits<T> *__restrict__ sorted_val,
                                                       const uint64_t *__restrict__ headscan, const uint64_t *__restrict__ head_pos, uint64_t nprod,
                                                       const int64_t *__restrict__ a_rowptr, const uint64_t *__restrict__ wscan,
                                                       const uint32_t *__restrict__ long_rows, const uint64_t *__restrict__ loff, int colbits,
                                                       uint64_t p0, uint32_t *__restrict__ tcol, ValueBits<T> *__restrict__ tval) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    constexpr uint64_t kWaveRun = 64;
    const uint64_t nruns = headscan[nprod];
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned lane = lane_id();
    const bool mine = r < nruns;
    uint64_t a = 0, e = 0;
    if (mine) { a = head_pos[r]; e = head_pos[r + 1]; }
    V acc = 0;
    const bool lng = mine && (e - a) > kWaveRun;
    if (mine && !lng) {
        acc = sorted_val[a];
        for (uint64_t u = a + 1; u < e; u++) acc = ewise_apply<ADD, T, V>(acc, sorted_val[u]);
    }
    uint64_t m = __ballot(lng);
    while (m) {
        const uint32_t j = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint64_t ja = wave_bcast(a, j), je = wave_bcast(e, j);
        V sum = 0;
        for (uint64_t b0 = ja; b0 < je; b0 += kWave) {
            const uint64_t x = b0 + lane;
            const V v = x < je ? sorted_val[x] : (V)0;
            const uint32_t cnt = (uint32_t)min((uint64_t)kWave, je - b0);
            uint32_t t0 = 0;
            if (b0 == ja) { sum = wave_bcast(v, 0u); t0 = 1; }   // the fold starts AS the first product
            for (uint32_t t = t0; t < cnt; t++) sum = ewise_apply<ADD, T, V>(sum, wave_bcast(v, t));
        }
        if (lane == j) acc = sum;
    }
    if (!mine) return;
    const uint64_t k = key[a];
    const uint64_t h = k >> colbits;
    const uint64_t o = wscan[a_rowptr[long_rows[h]]] - p0 + (r - headscan[loff[h]]);
    tcol[o] = (uint32_t)(k & ((1ull << colbits) - 1ull));
    tval[o] = acc;
}
__global__ __launch_bounds__(256) void mxm_long_counts_kernel(const uint32_t *__restrict__ long_rows, const uint64_t *__restrict__ loff, uint32_t nlong,
                                                              const uint64_t *__restrict__ headscan, uint32_t *__restrict__ cnt) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nlong) return;
    cnt[long_rows[h]] = (uint32_t)(headscan[loff[h + 1]] - headscan[loff[h]]);
}

// ---- output: the slots' entries to the batch's output, a lane per output entry ------------------------------------------------
// bptr: the exclusive scan of the batch's row counts (nrows + 1 entries)
template <class V>
__global__ __launch_bounds__(256) void mxm_gather_kernel(const int64_t *__restrict__ a_rowptr, const uint64_t *__restrict__ wscan, uint64_t r0,
                                                         uint64_t nrows, uint64_t p0, const uint64_t *__restrict__ bptr, uint64_t nnz,
                                                         const uint32_t *__restrict__ tcol, const V *__restrict__ tval,
                                                         uint32_t *__restrict__ out_col, V *__restrict__ out_val) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nnz) return;
    const uint64_t x = upper_bound_dev(bptr, 0, nrows + 1, o) - 1;
    const uint64_t src = wscan[a_rowptr[r0 + x]] - p0 + (o - bptr[x]);
    out_col[o] = tcol[src];
    out_val[o] = tval[src];
}

}  // namespace osp
