// osp_assign.h -- out = c with the region (rows, cols) assigned from a: the kernels of osp_csr_assign
// (include/outerspace_spgemm_assign.h), written for gfx950 (wave64).  DESIGN.md section 29.
//
// a's entry (i, k) lands at (rows[i], cols[k]) of out.  embed(a), the M x N matrix with a in its place, is never stored: the
// row map R (R[r] = i + 1 where rows[i] == r, else 0), the column bitmap of osp_extract.h with its ranks, and the lists
// themselves translate a coordinate in either direction where it is needed.  Both operands are sorted and, through R, row
// aligned, so nothing is sorted here: this is osp_ewise.h's union with a translation in front of every search.
//   1. row map: a thread per rows[i]: an integer compare-and-swap from 0 claims R[rows[i]]; a claimed word (a repeated row)
//               or an index >= M raises the error word instead and is never an address
//   2. col map: extract_colmap_kernel and the scan of its words' popcounts, as they stand
//   3. flag:    over the entries of c, ONE bit per entry: X[p] = "c's side does not write this entry".  Without accum that is
//               every entry of the region (row listed and column listed); with accum only those of the region that a holds
//               too, which a's side writes as op(c, a).  Whether a holds it is a bisection for rank(column) in a's row.  The
//               other of the two counts (the region under accum, the hits without) is a ballot's popcount added to a counter.
//   4. scan of the words' popcounts; the call's ONE read-back: the error word, the number of set bits and the counter
//   5. lengths: a thread per row of out: c's length minus its set bits plus a's row length where the row is listed; their
//               scan is out's row pointer
//   6. c side:  an entry without its bit goes to out.rowptr[r] + (its rank among its row's kept entries) + (a's entries of the
//               row before it: the lower bound of rank(column) in a's row)
//   7. a side:  an entry goes to out.rowptr[r] + (its place in a's row) + (c's kept entries of the row before it: the lower
//               bound q of cols[k] in c's row, minus the set bits of the row before q); its value is op(c[q], a) on a hit
//               under accum, a's bits otherwise
// Work is cut by ENTRIES (kCompactChunk a workgroup) in passes 3, 6 and 7; an entry's row is chunk_entries_and_rows'
// bisection, a lane's searches advance together.  Every output position is a function of bit arrays, scans and bisections
// alone: the only atomics are the integer ones of passes 1 to 3, whose results do not depend on any order.  The accum
// operator is a template parameter.
#pragma once
#include "osp_ewise.h"
#include "osp_extract.h"

namespace osp {

constexpr uint32_t kAssignBadRow = 1u, kAssignBadCol = kExtractBadCol, kAssignRepeatedRow = 4u;   // bits of the error word

// The two translations of a call.  rmap: null for the identity (no row list); colbits: null when every column is listed.
struct AssignMaps {
    const uint32_t *rmap;      // M words: i + 1 where rows[i] == r
    const uint32_t *rows;      // the row list (null: identity)
    const uint64_t *colbits;   // the column bitmap, cpos its scan
    const uint32_t *cpos;
    const uint32_t *cols;      // the column list (null: identity)
    // 1 + a's row for row r of c, 0 when r is not listed
    __device__ __forceinline__ uint32_t a_row_plus1(uint32_t r) const { return rmap ? rmap[r] : r + 1; }
    __device__ __forceinline__ bool col_listed(uint32_t j) const { return colbits ? extract_col_kept(colbits, j) : true; }
    // the number of listed columns below j: a's column for a listed j
    __device__ __forceinline__ uint32_t col_rank(uint32_t j) const {
        return colbits ? cpos[j >> 6] + (uint32_t)__popcll(colbits[j >> 6] & ((1ull << (j & 63)) - 1ull)) : j;
    }
    __device__ __forceinline__ uint32_t c_row(uint32_t i) const { return rows ? rows[i] : i; }
    __device__ __forceinline__ uint32_t c_col(uint32_t k) const { return cols ? cols[k] : k; }
};

// ---- 1: the row map ----------------------------------------------------------------------------------------------------------
// rmap: M words, zeroed by the caller
__global__ __launch_bounds__(256) void assign_rowmap_kernel(const uint32_t *__restrict__ rows, uint64_t n_rows, uint64_t M, uint32_t *rmap,
                                                            uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint64_t r = rows[i];
    if (r >= M) atomicOr(err, kAssignBadRow);
    else if (atomicCAS(&rmap[r], 0u, (uint32_t)i + 1u) != 0u) atomicOr(err, kAssignRepeatedRow);   // (n_rows < 2^32 - 1)
}

// The lane's entries of c's chunk at `base` searched in a: p[k] the entry, j[k] its column, row[k] its row; for an entry of a
// listed row, q[k] is the absolute lower bound of rank(j[k]) in a's row and a_begin[k] that row's first position; listed[k]
// says so.  REGION_ONLY: only entries whose column is listed too are searched (the others keep q == a_begin).
// (positions in a and row numbers are kept in 32 bits: M and nnz(a) are below 2^32)
template <bool REGION_ONLY>
__device__ __forceinline__ void assign_chunk_search_a(const int64_t *__restrict__ c_rowptr, const uint32_t *__restrict__ c_col, uint64_t M,
                                                      uint64_t nnz_c, uint64_t base, const AssignMaps &mp, const int64_t *__restrict__ a_rowptr,
                                                      const uint32_t *__restrict__ a_col, int64_t (&p)[kCompactRounds],
                                                      uint32_t (&j)[kCompactRounds], uint32_t (&row)[kCompactRounds],
                                                      uint32_t (&q)[kCompactRounds], uint32_t (&a_begin)[kCompactRounds],
                                                      bool (&listed)[kCompactRounds], bool (&hit)[kCompactRounds]) {
    uint32_t hi[kCompactRounds], end[kCompactRounds], x[kCompactRounds];
    chunk_entries_and_rows(c_rowptr, c_col, M, nnz_c, base, p, j, row, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        row[k] -= 1;
        const bool valid = (uint64_t)p[k] < nnz_c;
        const uint32_t i1 = valid ? mp.a_row_plus1(row[k]) : 0u;
        listed[k] = i1 != 0u;
        if (REGION_ONLY) listed[k] = listed[k] && mp.col_listed(j[k]);
        q[k] = listed[k] ? (uint32_t)a_rowptr[i1 - 1] : 0u;
        hi[k] = listed[k] ? (uint32_t)a_rowptr[i1] : 0u;
        a_begin[k] = q[k];
        end[k] = hi[k];
        x[k] = listed[k] ? mp.col_rank(j[k]) : 0u;
    }
    bisect_together<false>(a_col, q, hi, x);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) hit[k] = q[k] < end[k] && a_col[q[k]] == x[k];
}

// ---- 3: one bit per entry of c: c's side does not write it -------------------------------------------------------------------
// other: the count of the verdict that is NOT stored (ACCUM: entries of the region; else: entries of the region that a holds)
template <bool ACCUM>
__global__ __launch_bounds__(kCompactThreads) void assign_flag_kernel(const int64_t *__restrict__ c_rowptr, const uint32_t *__restrict__ c_col,
                                                                       uint64_t M, uint64_t nnz_c, AssignMaps mp,
                                                                       const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col,
                                                                       uint64_t *__restrict__ bits, unsigned long long *other) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_c) return;
    int64_t p[kCompactRounds];
    uint32_t j[kCompactRounds], row[kCompactRounds], q[kCompactRounds], a_begin[kCompactRounds];
    bool region[kCompactRounds], hit[kCompactRounds];
    assign_chunk_search_a<true>(c_rowptr, c_col, M, nnz_c, base, mp, a_rowptr, a_col, p, j, row, q, a_begin, region, hit);
    uint32_t n_other = 0;
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const bool both = region[k] && hit[k];
        store_verdicts(ACCUM ? both : region[k], (uint64_t)p[k], nnz_c, bits);
        n_other += (uint32_t)__popcll(__ballot(ACCUM ? region[k] : both));
    }
    if (lane_id() == 0 && n_other) atomicAdd(other, (unsigned long long)n_other);
}

// ---- 5: the length of every row of out ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assign_len_kernel(const int64_t *__restrict__ c_rowptr, uint64_t M, AssignMaps mp,
                                                         const int64_t *__restrict__ a_rowptr, const uint64_t *__restrict__ bits,
                                                         const uint64_t *__restrict__ pos, uint32_t *__restrict__ len) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const uint64_t b = (uint64_t)c_rowptr[r], e = (uint64_t)c_rowptr[r + 1];
    uint64_t l = e - b;
    const uint32_t i1 = mp.a_row_plus1((uint32_t)r);
    if (i1) l = l - (ewise_hits_before(bits, pos, e) - ewise_hits_before(bits, pos, b)) + (uint64_t)(a_rowptr[i1] - a_rowptr[i1 - 1]);
    len[r] = (uint32_t)l;   // (out holds fewer than 2^32 entries: the entry point checks the operands' sum)
}

// ---- 6: c's side ---------------------------------------------------------------------------------------------------------------
template <class V>
__global__ __launch_bounds__(kCompactThreads) void assign_write_c_kernel(const int64_t *__restrict__ c_rowptr, const uint32_t *__restrict__ c_col,
                                                                          const V *__restrict__ c_val, uint64_t M, uint64_t nnz_c, AssignMaps mp,
                                                                          const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col,
                                                                          const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                                          const int64_t *__restrict__ out_rowptr, uint32_t *__restrict__ out_col,
                                                                          V *__restrict__ out_val) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_c) return;
    int64_t p[kCompactRounds];
    uint32_t j[kCompactRounds], row[kCompactRounds], q[kCompactRounds], a_begin[kCompactRounds];
    bool listed[kCompactRounds], hit[kCompactRounds];
    assign_chunk_search_a<false>(c_rowptr, c_col, M, nnz_c, base, mp, a_rowptr, a_col, p, j, row, q, a_begin, listed, hit);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if ((uint64_t)p[k] >= nnz_c) continue;
        const uint64_t word = bits[p[k] >> 6];
        if ((word >> (p[k] & 63)) & 1ull) continue;   // deleted, or a's side writes this coordinate
        const uint64_t b = (uint64_t)c_rowptr[row[k]];
        uint64_t o = (uint64_t)out_rowptr[row[k]] + ((uint64_t)p[k] - b);
        if (listed[k]) {   // (an untouched row has no set bit and no entry of a)
            const uint64_t removed = pos[p[k] >> 6] + (uint64_t)__popcll(word & ((1ull << (p[k] & 63)) - 1ull)) - ewise_hits_before(bits, pos, b);
            o = o - removed + (uint64_t)(q[k] - a_begin[k]);
        }
        out_col[o] = j[k];
        out_val[o] = c_val[p[k]];
    }
}

// ---- 7: a's side ---------------------------------------------------------------------------------------------------------------
// OP: an EW_* operator, or a negative value for no accum (a's bits everywhere)
template <class T, int OP>
__global__ __launch_bounds__(kCompactThreads) void assign_write_a_kernel(
    const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col, const ValueBits<T> *__restrict__ a_val, uint64_t m, uint64_t nnz_a,
    AssignMaps mp, const int64_t *__restrict__ c_rowptr, const uint32_t *__restrict__ c_col, const ValueBits<T> *__restrict__ c_val,
    const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos, const int64_t *__restrict__ out_rowptr, uint32_t *__restrict__ out_col,
    ValueBits<T> *__restrict__ out_val) {
    typedef ValueBits<T> V;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_a) return;
    int64_t p[kCompactRounds];
    uint32_t j[kCompactRounds], i[kCompactRounds], q[kCompactRounds], hi[kCompactRounds], end[kCompactRounds], r[kCompactRounds];
    chunk_entries_and_rows(a_rowptr, a_col, m, nnz_a, base, p, j, i, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        i[k] -= 1;
        const bool valid = (uint64_t)p[k] < nnz_a;
        r[k] = valid ? mp.c_row(i[k]) : 0u;
        j[k] = valid ? mp.c_col(j[k]) : 0u;
        q[k] = valid ? (uint32_t)c_rowptr[r[k]] : 0u;
        hi[k] = valid ? (uint32_t)c_rowptr[r[k] + 1] : 0u;
        end[k] = hi[k];
    }
    bisect_together<false>(c_col, q, hi, j);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if ((uint64_t)p[k] >= nnz_a) continue;
        const uint64_t b = (uint64_t)c_rowptr[r[k]];
        const uint64_t kept_before = ((uint64_t)q[k] - b) - (ewise_hits_before(bits, pos, (uint64_t)q[k]) - ewise_hits_before(bits, pos, b));
        const uint64_t o = (uint64_t)out_rowptr[r[k]] + ((uint64_t)p[k] - (uint64_t)a_rowptr[i[k]]) + kept_before;
        V v = a_val[p[k]];
        if constexpr (OP >= 0) {
            if (q[k] < end[k] && c_col[q[k]] == j[k]) v = ewise_apply<OP, T, V>(c_val[q[k]], v);
        }
        out_col[o] = j[k];
        out_val[o] = v;
    }
}

}  // namespace osp
