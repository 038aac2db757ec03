// osp_apply_mask.h -- the mask filter C<M> / C<¬M> of a CSR result (osp_csr_apply_mask,
// include/outerspace_spgemm_apply_mask.h), written for gfx950 (wave64).  DESIGN.md section 11.
//
// Keep the entries of `in` whose coordinate is (keep sense) or is not (complement sense) in a CSR pattern of the same shape.
// Work is cut by ENTRIES of `in`, never by rows: a frontier product has a handful of rows of up to N entries, an ordinary
// product millions of short ones, and both take the same path.
//   1. flag:   one workgroup per chunk of kAmChunk consecutive entries (a chunk may span rows), kAmRounds entries a lane.
//              The chunk's first and last row are found once; an entry's row is a bisection between them (none when the
//              chunk lies inside one row), its membership a bisection for its column in that row of the mask.  A lane's
//              kAmRounds searches advance together, one step of each per trip, so that many loads are in flight per lane:
//              the searches are chains of dependent loads and nothing else.  The 64 verdicts of a wave become ONE word of a
//              bit array (ballot): entry p is bit p & 63 of word p >> 6.
//   2. scan:   the library's exclusive scan over the words' popcounts: pos[w] = kept entries before entry 64 w.
//   3. write:  entry p with its bit set goes to pos[p >> 6] + popcount(word below bit p & 63): a lane per entry, values moved
//              as integers of their width; and the output's row pointer is the same expression evaluated at in.rowptr[i].
// Every output position is a function of the bit array alone: no atomics, and nothing depends on the order of processing.
// (Narrowing the search to the window of the mask row that a wave's run of same-row entries can hit was built and measured:
// MEASUREMENTS.md section 0d.  It lost on the frontier shape and changed nothing on short rows, so it is not here.)
#pragma once
#include "osp_kernels.h"
#include "osp_prims.h"

namespace osp {

constexpr int kAmThreads = 256;
constexpr int kAmRounds = 8;
constexpr uint64_t kAmChunk = (uint64_t)kAmThreads * kAmRounds;   // 2048 entries of `in` per workgroup

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

// ---- pass 1: one verdict bit per entry ------------------------------------------------------------------------------------
// (positions in the mask and row numbers are kept in 32 bits: M and nnz(mask) are below 2^32)
__global__ __launch_bounds__(kAmThreads) void apply_mask_flag_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                      uint64_t M, uint64_t nnz, const int64_t *__restrict__ m_rowptr,
                                                                      const uint32_t *__restrict__ m_col, int complement,
                                                                      uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kAmChunk;
    if (base >= nnz) return;
    const uint64_t last = (base + kAmChunk < nnz ? base + kAmChunk : nnz) - 1;
    // the rows of the chunk's first and last entry (the last row r with rowptr[r] <= p holds entry p; same addresses in
    // every lane)
    const uint32_t r_first = (uint32_t)(upper_bound_dev(rowptr, 0, M + 1, (int64_t)base) - 1);
    const uint32_t r_last = (uint32_t)(upper_bound_dev(rowptr, (uint64_t)r_first + 1, M + 1, (int64_t)last) - 1);
    uint32_t lo[kAmRounds], hi[kAmRounds], j[kAmRounds];
    int64_t p[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        p[k] = (int64_t)(base + (uint64_t)k * kAmThreads + threadIdx.x);
        const bool valid = (uint64_t)p[k] < nnz;
        j[k] = valid ? col[p[k]] : 0u;
        lo[k] = r_first + 1;                      // the row is the last index in [r_first, r_last] with rowptr[.] <= p
        hi[k] = valid ? r_last + 1 : r_first + 1;
    }
    if (r_first != r_last) bisect_together<true>(rowptr, lo, hi, p);
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const uint32_t r = lo[k] - 1;
        const bool valid = (uint64_t)p[k] < nnz;
        lo[k] = valid ? (uint32_t)m_rowptr[r] : 0u;
        hi[k] = valid ? (uint32_t)m_rowptr[r + 1] : 0u;
    }
    uint32_t end[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) end[k] = hi[k];
    bisect_together<false>(m_col, lo, hi, j);
    bool keep[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const bool member = lo[k] < end[k] && m_col[lo[k]] == j[k];
        keep[k] = (uint64_t)p[k] < nnz && member != (complement != 0);
    }
    const unsigned lane = lane_id();
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const uint64_t word = __ballot(keep[k]);
        if (lane == 0 && (uint64_t)p[k] < nnz) bits[p[k] >> 6] = word;   // (lane 0 holds the word's first entry)
    }
}

// ---- pass 3: the kept entries at their positions, the row pointers -------------------------------------------------------
// V: an unsigned integer of the value's width (values are moved, never computed)
template <class V>
__global__ __launch_bounds__(256) void apply_mask_write_kernel(const uint32_t *__restrict__ col, const V *__restrict__ val, uint64_t nnz,
                                                               const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                               uint32_t *__restrict__ out_col, V *__restrict__ out_val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t word = bits[p >> 6];
    if ((word >> (p & 63)) & 1ull) {
        const uint64_t o = pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull));
        out_col[o] = col[p];
        out_val[o] = val[p];
    }
}
// out_rowptr[i] = kept entries before entry in.rowptr[i], for i in [0, M]
__global__ __launch_bounds__(256) void apply_mask_rowptr_kernel(const int64_t *__restrict__ rowptr, uint64_t M, const uint64_t *__restrict__ bits,
                                                                const uint64_t *__restrict__ pos, int64_t *__restrict__ out_rowptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    const uint64_t p = (uint64_t)rowptr[i];
    uint64_t o = pos[p >> 6];
    if (p & 63) o += (uint64_t)__popcll(bits[p >> 6] & ((1ull << (p & 63)) - 1ull));   // (p & 63 == 0: the word may not exist)
    out_rowptr[i] = (int64_t)o;
}

}  // namespace osp
