// osp_select.h -- the entry filter of a CSR result (osp_csr_select, include/outerspace_spgemm_select.h), written for gfx950
// (wave64).  DESIGN.md section 12.
//
// Keep the entries of `in` whose value passes a comparison with a threshold, or whose column lies on one side of the diagonal
// row + diag.  The flag pass of osp_compact.h's three passes, one workgroup per chunk of kCompactChunk consecutive entries,
// kCompactRounds entries a lane.  A VALUE predicate is a pure stream over `vals`: a lane's kCompactRounds loads are issued
// before any is compared, no row is looked up, colidx and rowptr are not touched.  A POSITION predicate needs the entry's
// row: chunk_entries_and_rows.  The predicate is a template parameter: there is no branch on it in the kernel.  The write
// pass stores a constant in place of the values (compact_write_kernel<V, true>) when the caller asks for one.
#pragma once
#include "osp_compact.h"

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
__global__ __launch_bounds__(kCompactThreads) void select_flag_value_kernel(const T *__restrict__ val, uint64_t nnz, double threshold,
                                                                             uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    T v[kCompactRounds];
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kCompactThreads + threadIdx.x;
        v[k] = p < nnz ? val[p] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kCompactThreads + threadIdx.x;
        store_verdicts(p < nnz && select_compare<OP, double>((double)v[k], threshold), p, nnz, bits);
    }
}

// ---- pass 1, position predicates: col[p] OP row(p) + diag -------------------------------------------------------------------
// (row numbers are kept in 32 bits: M is below 2^32; diag was clamped by the host to +-2^33, beyond every col - row, so
// row + diag cannot overflow)
template <int OP>
__global__ __launch_bounds__(kCompactThreads) void select_flag_position_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                                uint64_t M, uint64_t nnz, int64_t diag, uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const bool valid = (uint64_t)p[k] < nnz;
        store_verdicts(valid && select_compare<OP, int64_t>((int64_t)j[k], (int64_t)(lo[k] - 1) + diag), (uint64_t)p[k], nnz, bits);
    }
}

}  // namespace osp
