// osp_compact.h -- compaction of a CSR by one verdict bit per entry, written for gfx950 (wave64): what the filters of
// osp_apply_mask.h and osp_select.h share.  DESIGN.md sections 11 and 12.
//
// Work is cut by ENTRIES of `in`, never by rows: a frontier product has a handful of rows of up to N entries, an ordinary
// product millions of short ones, and both take the same path.
//   1. flag:   one workgroup per chunk of kCompactChunk consecutive entries (a chunk may span rows), kCompactRounds entries a
//              lane.  The filter's own kernel decides; the 64 verdicts of a wave become ONE word of a bit array (ballot):
//              entry p is bit p & 63 of word p >> 6 (store_verdicts).  A filter that needs an entry's row gets it from
//              chunk_entries_and_rows.
//   2. scan:   the library's exclusive scan over the words' popcounts (LoadPopc64): pos[w] = kept entries before entry 64 w.
//   3. write:  entry p with its bit set goes to pos[p >> 6] + popcount(word below bit p & 63): a lane per entry, values moved
//              as integers of their width (or a constant stored in their place); and the output's row pointer is the same
//              expression evaluated at in.rowptr[i].
// Every output position is a function of the bit array alone: no atomics, and nothing depends on the order of processing.
#pragma once
#include "osp_kernels.h"
#include "osp_prims.h"

namespace osp {

constexpr int kCompactThreads = 256;
constexpr int kCompactRounds = 8;
constexpr uint64_t kCompactChunk = (uint64_t)kCompactThreads * kCompactRounds;   // 2048 entries of `in` per workgroup

struct LoadPopc64 {
    const uint64_t *w;
    __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)__popcll(w[i]); }
};

// R bisections side by side: on return lo[k] is the first index in [lo[k], hi[k]) whose element is >= x[k] (UPPER: > x[k]),
// or hi[k].  Every trip issues the loads of all searches still open before any of them is used.
template <bool UPPER, int R, class T, class X>
__device__ __forceinline__ void bisect_together(const T *__restrict__ a, uint32_t (&lo)[R], uint32_t (&hi)[R], const X (&x)[R]) {
    for (;;) {
        T v[R];
        uint32_t mid[R];
        bool open = false;
#pragma unroll
        for (int k = 0; k < R; k++) {
            mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
            if (lo[k] < hi[k]) {
                v[k] = a[mid[k]];
                open = true;
            }
        }
        if (!open) break;
#pragma unroll
        for (int k = 0; k < R; k++) {
            if (lo[k] < hi[k]) {
                const bool right = UPPER ? (X)v[k] <= x[k] : (X)v[k] < x[k];
                if (right) lo[k] = mid[k] + 1; else hi[k] = mid[k];
            }
        }
    }
}

// ---- pass 1: what the flag kernels share -----------------------------------------------------------------------------------
// The lane's entries of the chunk that begins at entry `base` (< nnz), with their columns and rows: p[k] is the entry of
// round k, j[k] its column (0 past the end), lo[k] - 1 its row.  The chunk's first and last row are found once; an entry's
// row is a bisection between them (none when the chunk lies inside one row), all of a lane's searches advancing together.
// (row numbers are kept in 32 bits: M is below 2^32)
__device__ __forceinline__ void chunk_entries_and_rows(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, uint64_t M,
                                                       uint64_t nnz, uint64_t base, int64_t (&p)[kCompactRounds],
                                                       uint32_t (&j)[kCompactRounds], uint32_t (&lo)[kCompactRounds],
                                                       uint32_t (&hi)[kCompactRounds]) {
    const uint64_t last = (base + kCompactChunk < nnz ? base + kCompactChunk : nnz) - 1;
    // the rows of the chunk's first and last entry (the last row r with rowptr[r] <= p holds entry p; same addresses in
    // every lane)
    const uint32_t r_first = (uint32_t)(upper_bound_dev(rowptr, 0, M + 1, (int64_t)base) - 1);
    const uint32_t r_last = (uint32_t)(upper_bound_dev(rowptr, (uint64_t)r_first + 1, M + 1, (int64_t)last) - 1);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        p[k] = (int64_t)(base + (uint64_t)k * kCompactThreads + threadIdx.x);
        const bool valid = (uint64_t)p[k] < nnz;
        j[k] = valid ? col[p[k]] : 0u;
        lo[k] = r_first + 1;                      // the row is the last index in [r_first, r_last] with rowptr[.] <= p
        hi[k] = valid ? r_last + 1 : r_first + 1;
    }
    if (r_first != r_last) bisect_together<true>(rowptr, lo, hi, p);
}

// 64 verdicts -> one word: `keep` is the verdict on entry p (false past the end); lane 0 holds the word's first entry
__device__ __forceinline__ void store_verdicts(bool keep, uint64_t p, uint64_t nnz, uint64_t *__restrict__ bits) {
    const uint64_t word = __ballot(keep);
    if (lane_id() == 0 && p < nnz) bits[p >> 6] = word;
}

// ---- pass 3: the kept entries at their positions, the row pointers -------------------------------------------------------
// V: an unsigned integer of the value's width (values are moved, never computed).  FILL: `in`'s values are not read, every
// kept entry gets the constant's bits.
template <class V, bool FILL>
__global__ __launch_bounds__(256) void compact_write_kernel(const uint32_t *__restrict__ col, const V *__restrict__ val, uint64_t nnz,
                                                            const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos, V fill,
                                                            uint32_t *__restrict__ out_col, V *__restrict__ out_val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t word = bits[p >> 6];
    if ((word >> (p & 63)) & 1ull) {
        const uint64_t o = pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull));
        out_col[o] = col[p];
        out_val[o] = FILL ? fill : val[p];
    }
}
// out_rowptr[i] = kept entries before entry in.rowptr[i], for i in [0, M]
__global__ __launch_bounds__(256) void compact_rowptr_kernel(const int64_t *__restrict__ rowptr, uint64_t M, const uint64_t *__restrict__ bits,
                                                             const uint64_t *__restrict__ pos, int64_t *__restrict__ out_rowptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    const uint64_t p = (uint64_t)rowptr[i];
    uint64_t o = pos[p >> 6];
    if (p & 63) o += (uint64_t)__popcll(bits[p >> 6] & ((1ull << (p & 63)) - 1ull));   // (p & 63 == 0: the word may not exist)
    out_rowptr[i] = (int64_t)o;
}

}  // namespace osp
