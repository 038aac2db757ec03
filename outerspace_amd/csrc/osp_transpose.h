// osp_transpose.h -- the transpose of a CSR result (osp_csr_transpose, include/outerspace_spgemm_transpose.h), written for
// gfx950 (wave64).  DESIGN.md section 16.
//
// The output is a stable counting sort of in's entries by column: the input is in row order, so a stable sort leaves
// ascending rows inside every column, which are the ascending columns of the output's rows.  Two paths:
//
//   row mask   in has at most 64 rows (a frontier, a batch of sources).  One 64-bit word per column of in:
//              tr_rowmask_kernel ORs bit i into mask[j] for every entry (i, j) -- an integer atomic, order-free, and every
//              bit is set once because a row holds a column once; the library's exclusive scan of the words' popcounts IS
//              the output's row pointer; tr_place_kernel puts entry (i, j) at rowptr[j] + popcount(mask[j] below bit i).
//              Both kernels are cut by entries (chunk_entries_and_rows): one row of 2^19 entries costs what 64 short ones cost.
//   sort       everything else: device_sort_rows (osp_sort.h) on in's column array as it stands.  Its first pass makes the
//              positions, its last pass hands (t, column, position) to TrEpilogue, which writes the output's column (in's
//              row) and value at t and the sorted column for ingest_ptr_kernel's bisections: neither keys nor positions are
//              materialised at either end.  What the epilogue needs at a position -- the entry's row and value -- comes
//              PACKED: tr_pack_kernel writes one (row, value bits) record per entry before the sort (8 bytes at f32, 16 at
//              f64), so the last pass does ONE gather per element; or UNPACKED: it bisects in's row pointer with the
//              position and gathers the value by itself (no pack kernel, no record array).
//
// Values are moved as integers of their width.  No float atomics, no waiting between workgroups, no scratch.
#pragma once
#include "osp_compact.h"
#include "osp_ewise.h"
#include "osp_sort.h"

namespace osp {

constexpr uint64_t kTrMaskRows = 64;   // the row-mask path: a row is a bit of a 64-bit word

// ---- row-mask path ------------------------------------------------------------------------------------------------------------
// (a column beyond N is not an entry of a valid result; it is skipped here and in tr_place_kernel rather than written past
// the mask)
__global__ __launch_bounds__(kCompactThreads) void tr_rowmask_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                     uint64_t M, uint64_t N, uint64_t nnz,
                                                                     unsigned long long *__restrict__ mask) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint32_t i = lo[k] - 1;
        if ((uint64_t)p[k] < nnz && j[k] < N && i < kTrMaskRows) atomicOr(&mask[j[k]], 1ull << i);
    }
}
// entry (i, j) -> out[rowptr_out[j] + the rows below i that hold column j]; the column written is i
template <class V>
__global__ __launch_bounds__(kCompactThreads) void tr_place_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                   const V *__restrict__ val, uint64_t M, uint64_t N, uint64_t nnz,
                                                                   const uint64_t *__restrict__ mask, const int64_t *__restrict__ out_rowptr,
                                                                   uint32_t *__restrict__ out_col, V *__restrict__ out_val) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint32_t i = lo[k] - 1;
        if ((uint64_t)p[k] < nnz && j[k] < N && i < kTrMaskRows) {
            const uint64_t o = (uint64_t)out_rowptr[j[k]] + (uint64_t)__popcll(mask[j[k]] & ((1ull << i) - 1ull));
            out_col[o] = i;
            out_val[o] = val[p[k]];
        }
    }
}

// ---- sort path ----------------------------------------------------------------------------------------------------------------
// one record per entry: (row, value bits) -- uint2 at 4-byte values, uint4 (row, 0, low word, high word) at 8-byte ones
template <class V> struct TrRecord;
template <> struct TrRecord<uint32_t> {
    typedef uint2 type;
    static __device__ __forceinline__ uint2 make(uint32_t row, uint32_t v) { return make_uint2(row, v); }
    static __device__ __forceinline__ uint32_t value(const uint2 &r) { return r.y; }
};
template <> struct TrRecord<uint64_t> {
    typedef uint4 type;
    static __device__ __forceinline__ uint4 make(uint32_t row, uint64_t v) { return make_uint4(row, 0u, (uint32_t)v, (uint32_t)(v >> 32)); }
    static __device__ __forceinline__ uint64_t value(const uint4 &r) { return (uint64_t)r.z | ((uint64_t)r.w << 32); }
};

template <class V>
__global__ __launch_bounds__(kCompactThreads) void tr_pack_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                  const V *__restrict__ val, uint64_t M, uint64_t nnz,
                                                                  typename TrRecord<V>::type *__restrict__ rec) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++)
        if ((uint64_t)p[k] < nnz) rec[p[k]] = TrRecord<V>::make(lo[k] - 1, val[p[k]]);
}

// the sort's last pass: element t of the output is in's entry `pos`, whose column is `column`
template <class V, bool PACKED>
struct TrEpilogue {
    const typename TrRecord<V>::type *rec;   // PACKED
    const int64_t *rowptr;                   // !PACKED: in's row pointer, M + 1 entries
    const V *val;                            // !PACKED: in's values
    uint64_t M;
    uint32_t *out_col, *sorted_cols;
    V *out_val;
    __device__ void operator()(uint64_t t, uint32_t column, uint32_t pos) const {
        if (PACKED) {
            const typename TrRecord<V>::type r = rec[pos];
            out_col[t] = r.x;
            out_val[t] = TrRecord<V>::value(r);
        } else {
            out_col[t] = (uint32_t)(upper_bound_dev(rowptr, 0, M + 1, (int64_t)pos) - 1);
            out_val[t] = val[pos];
        }
        sorted_cols[t] = column;
    }
};

}  // namespace osp
