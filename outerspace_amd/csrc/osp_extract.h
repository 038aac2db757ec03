// osp_extract.h -- the submatrix out = in(rows, cols) of a CSR result, renumbered, written for gfx950 (wave64): the kernels of
// osp_csr_extract (include/outerspace_spgemm_extract.h).  DESIGN.md section 18.
//
// The GATHERED matrix G -- the rows of `in` the row list names, in list order, duplicates included -- is never stored: its
// row pointer g (the scan of the listed rows' lengths) says where entry e of G lies in `in`:
//     row r = the last index with g[r] <= e,      source position = in.rowptr[rows[r]] + (e - g[r]).
// The column list becomes a bitmap of N bits and the scan of its words' popcounts (cpos), so column j is kept when its bit
// is set and its new index is cpos[j >> 6] + popcount(word below bit j & 63): osp_compact.h's expression, on columns.
//   1. lengths: a thread per rows[i]; an index >= M has length 0 and raises the error word, it is never an address
//   2. map:     a thread per cols[t] ORs its bit into the bitmap; a column >= N or not above its predecessor raises the
//               error word instead and sets no bit
//   3. flag:    osp_compact.h's pass 1 over the entries of G: one verdict bit per entry (only with a column list)
//   4. scan, row pointer: osp_compact.h's, with g in the row pointer's place
//   5. write:   a kept entry goes to the compaction's position (without a column list: its own position in G), its column
//               to its rank in the map, its value bits are moved
// Work is cut by ENTRIES of G, kCompactChunk a workgroup, as in osp_compact.h: a chunk's first and last row are found once,
// an entry's row is a bisection between them, all of a lane's searches advancing together.  Pass 5 searches again rather than
// keep a row or a source position per entry from pass 3: that would be 4 to 8 bytes written and read back per gathered entry
// where the search reads a few words of g that the whole chunk shares.
// Every output position is a function of the bit arrays alone: no float atomics, no order dependence, no waiting between
// workgroups; the one atomic is the integer OR of step 2.
#pragma once
#include "osp_compact.h"

namespace osp {

constexpr uint32_t kExtractBadRow = 1u, kExtractBadCol = 2u;   // bits of the error word

// ---- 1: the lengths of the listed rows -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void extract_len_kernel(const uint32_t *__restrict__ rows, uint64_t n_rows, const int64_t *__restrict__ rowptr,
                                                          uint64_t M, uint32_t *__restrict__ len, uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint64_t r = rows[i];
    uint32_t l = 0;
    if (r < M) l = (uint32_t)(rowptr[r + 1] - rowptr[r]);   // (a row holds fewer than 2^32 entries: the entry point checks nnz)
    else atomicOr(err, kExtractBadRow);
    len[i] = l;
}

// ---- 2: the column map -----------------------------------------------------------------------------------------------------------
// bits: (N + 63) / 64 words, zeroed by the caller.  dense (may be null): N words, dense[cols[t]] = t for the alternative map
// of OSP_EXTRACT_DENSE_MAP=1; only the words of kept columns are ever read.
__global__ __launch_bounds__(256) void extract_colmap_kernel(const uint32_t *__restrict__ cols, uint64_t n_cols, uint64_t N,
                                                             unsigned long long *bits, uint32_t *__restrict__ dense, uint32_t *err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cols) return;
    const uint64_t c = cols[t];
    if (c < N && (t == 0 || (uint64_t)cols[t - 1] < c)) {
        atomicOr(&bits[c >> 6], 1ull << (c & 63));
        if (dense) dense[c] = (uint32_t)t;
    } else {
        atomicOr(err, kExtractBadCol);
    }
}
__device__ __forceinline__ bool extract_col_kept(const uint64_t *__restrict__ colbits, uint32_t j) { return (colbits[j >> 6] >> (j & 63)) & 1ull; }

// The rows of a lane's entries of the chunk of G that begins at entry `base` (< nnz_g): on return lo[k] - 1 is the row of
// entry p[k] for every k with want[k]; the others are not searched.  chunk_entries_and_rows of osp_compact.h with g for the
// row pointer and without the column loads (a column of G is behind the row's source position).
__device__ __forceinline__ void extract_chunk_rows(const int64_t *__restrict__ g, uint64_t n_rows, uint64_t nnz_g, uint64_t base,
                                                   const int64_t (&p)[kCompactRounds], const bool (&want)[kCompactRounds],
                                                   uint32_t (&lo)[kCompactRounds], uint32_t (&hi)[kCompactRounds]) {
    const uint64_t last = (base + kCompactChunk < nnz_g ? base + kCompactChunk : nnz_g) - 1;
    const uint32_t r_first = (uint32_t)(upper_bound_dev(g, 0, n_rows + 1, (int64_t)base) - 1);
    const uint32_t r_last = (uint32_t)(upper_bound_dev(g, (uint64_t)r_first + 1, n_rows + 1, (int64_t)last) - 1);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        lo[k] = r_first + 1;
        hi[k] = want[k] ? r_last + 1 : r_first + 1;
    }
    if (r_first != r_last) bisect_together<true>(g, lo, hi, p);
}

// ---- 3: one verdict per entry of G: is its column in the map -----------------------------------------------------------------------
// ROWS: G is the gathered matrix (g, rows); else G is `in` itself and an entry's column is at its own position.
template <bool ROWS>
__global__ __launch_bounds__(kCompactThreads) void extract_flag_kernel(const int64_t *__restrict__ g, const uint32_t *__restrict__ rows,
                                                                       const int64_t *__restrict__ in_rowptr, const uint32_t *__restrict__ in_col,
                                                                       uint64_t n_rows, uint64_t nnz_g, const uint64_t *__restrict__ colbits,
                                                                       uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_g) return;
    int64_t p[kCompactRounds];
    bool valid[kCompactRounds];
    uint32_t lo[kCompactRounds], hi[kCompactRounds];
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        p[k] = (int64_t)(base + (uint64_t)k * kCompactThreads + threadIdx.x);
        valid[k] = (uint64_t)p[k] < nnz_g;
    }
    if constexpr (ROWS) extract_chunk_rows(g, n_rows, nnz_g, base, p, valid, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        bool keep = false;
        if (valid[k]) {
            int64_t src = p[k];
            if constexpr (ROWS) src = in_rowptr[rows[lo[k] - 1]] + (p[k] - g[lo[k] - 1]);
            keep = extract_col_kept(colbits, in_col[src]);
        }
        store_verdicts(keep, (uint64_t)p[k], nnz_g, bits);
    }
}

// ---- 5: the kept entries at their positions --------------------------------------------------------------------------------------
// V: an unsigned integer of the value's width.  COLS: bits / pos are the verdicts and their scan, colbits / cpos the map (dense:
// the alternative 4-byte map, or null); else every entry of G is kept at its own position with its own column.
template <class V, bool ROWS, bool COLS>
__global__ __launch_bounds__(kCompactThreads) void extract_write_kernel(const int64_t *__restrict__ g, const uint32_t *__restrict__ rows,
                                                                        const int64_t *__restrict__ in_rowptr, const uint32_t *__restrict__ in_col,
                                                                        const V *__restrict__ in_val, uint64_t n_rows, uint64_t nnz_g,
                                                                        const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                                        const uint64_t *__restrict__ colbits, const uint32_t *__restrict__ cpos,
                                                                        const uint32_t *__restrict__ dense, uint32_t *__restrict__ out_col,
                                                                        V *__restrict__ out_val) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_g) return;
    int64_t p[kCompactRounds];
    bool kept[kCompactRounds];
    uint64_t o[kCompactRounds];
    uint32_t lo[kCompactRounds], hi[kCompactRounds];
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        p[k] = (int64_t)(base + (uint64_t)k * kCompactThreads + threadIdx.x);
        kept[k] = (uint64_t)p[k] < nnz_g;
        o[k] = (uint64_t)p[k];
        if constexpr (COLS) {
            if (kept[k]) {
                const uint64_t word = bits[p[k] >> 6];
                kept[k] = (word >> (p[k] & 63)) & 1ull;
                o[k] = pos[p[k] >> 6] + (uint64_t)__popcll(word & ((1ull << (p[k] & 63)) - 1ull));
            }
        }
    }
    if constexpr (ROWS) extract_chunk_rows(g, n_rows, nnz_g, base, p, kept, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if (!kept[k]) continue;
        int64_t src = p[k];
        if constexpr (ROWS) src = in_rowptr[rows[lo[k] - 1]] + (p[k] - g[lo[k] - 1]);
        uint32_t j = in_col[src];
        if constexpr (COLS) {
            if (dense) j = dense[j];
            else j = cpos[j >> 6] + (uint32_t)__popcll(colbits[j >> 6] & ((1ull << (j & 63)) - 1ull));
        }
        out_col[o[k]] = j;
        out_val[o[k]] = in_val[src];
    }
}

}  // namespace osp
