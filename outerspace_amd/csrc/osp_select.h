// osp_select.h -- the entry filter of a CSR result (osp_csr_select, include/outerspace_spgemm_select.h), written for gfx950
// (wave64).  DESIGN.md section 12.
//
// Keep the entries of `in` whose value passes a comparison with a threshold, or whose column lies on one side of the diagonal
// row + diag.  The three passes of osp_apply_mask.h with another first pass:
//   1. flag:   one workgroup per chunk of kAmChunk consecutive entries, kAmRounds entries a lane, the 64 verdicts of a wave
//              become ONE word of a bit array (ballot): entry p is bit p & 63 of word p >> 6.
//              A VALUE predicate is a pure stream over `vals`: a lane's kAmRounds loads are issued before any is compared, no
//              row is looked up, colidx and rowptr are not touched.  A POSITION predicate needs the entry's row: the chunk's
//              first and last row are found once and the row is a bisection between them (bisect_together<true>, as
//              apply_mask_flag_kernel does; none when the chunk lies inside one row).
//              The predicate is a template parameter: there is no branch on it in the kernel.
//   2. scan:   the library's exclusive scan over the words' popcounts (LoadPopc64).
//   3. write:  apply_mask_write_kernel and apply_mask_rowptr_kernel as they are when the values are kept; select_fill_kernel,
//              which reads only colidx and stores a constant, when they are replaced.
// Every output position is a function of the bit array alone: no atomics, and nothing depends on the order of processing.
#pragma once
#include "osp_apply_mask.h"

namespace osp {

// (the values of osp_select_op_t)
enum { SEL_LT = 0, SEL_LE, SEL_GT, SEL_GE, SEL_EQ, SEL_NE, SEL_TRIL, SEL_TRIU, SEL_DIAG, SEL_OFFDIAG, SEL_OPS };

// x OP y with the operators of the language: on doubles these are the IEEE comparisons (false with a NaN on either side, NE
// true; -0.0 == +0.0), on int64 the signed ones
template <int OP, class X>
__device__ __forceinline__ bool select_compare(X x, X y) {
    switch (OP) {   // (OP is a constant: one case survives)
        case SEL_LT: return x < y;
        case SEL_LE: case SEL_TRIL: return x <= y;
        case SEL_GT: return x > y;
        case SEL_GE: case SEL_TRIU: return x >= y;
        case SEL_EQ: case SEL_DIAG: return x == y;
        default: return x != y;   // SEL_NE, SEL_OFFDIAG
    }
}

// ---- pass 1, value predicates: vals[p] OP threshold -------------------------------------------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(kAmThreads) void select_flag_value_kernel(const T *__restrict__ val, uint64_t nnz, double threshold,
                                                                        uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kAmChunk;
    if (base >= nnz) return;
    T v[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kAmThreads + threadIdx.x;
        v[k] = p < nnz ? val[p] : (T)0;
    }
    const unsigned lane = lane_id();
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kAmThreads + threadIdx.x;
        const uint64_t word = __ballot(p < nnz && select_compare<OP, double>((double)v[k], threshold));
        if (lane == 0 && p < nnz) bits[p >> 6] = word;   // (lane 0 holds the word's first entry)
    }
}

// ---- pass 1, position predicates: col[p] OP row(p) + diag -------------------------------------------------------------------
// (row numbers are kept in 32 bits: M is below 2^32; diag was clamped by the host to +-2^33, beyond every col - row, so
// row + diag cannot overflow)
template <int OP>
__global__ __launch_bounds__(kAmThreads) void select_flag_position_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                           uint64_t M, uint64_t nnz, int64_t diag, uint64_t *__restrict__ bits) {
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
    const unsigned lane = lane_id();
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const bool valid = (uint64_t)p[k] < nnz;
        const uint64_t word = __ballot(valid && select_compare<OP, int64_t>((int64_t)j[k], (int64_t)(lo[k] - 1) + diag));
        if (lane == 0 && valid) bits[p[k] >> 6] = word;
    }
}

// ---- pass 3 with a constant for the values: `in`'s values are not read ----------------------------------------------------
// V: an unsigned integer of the value's width (the constant's bits)
template <class V>
__global__ __launch_bounds__(256) void select_fill_kernel(const uint32_t *__restrict__ col, uint64_t nnz, const uint64_t *__restrict__ bits,
                                                          const uint64_t *__restrict__ pos, V fill, uint32_t *__restrict__ out_col,
                                                          V *__restrict__ out_val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t word = bits[p >> 6];
    if ((word >> (p & 63)) & 1ull) {
        const uint64_t o = pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull));
        out_col[o] = col[p];
        out_val[o] = fill;
    }
}

}  // namespace osp
