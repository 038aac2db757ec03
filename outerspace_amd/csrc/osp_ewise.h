// osp_ewise.h -- the element-wise union / intersection of two CSR results (osp_csr_ewise,
// include/outerspace_spgemm_ewise.h), written for gfx950 (wave64).  DESIGN.md section 13.
//
// Both operands are sorted and row-aligned, so nothing is sorted here: an entry's place in the output is its own position
// plus the number of the OTHER operand's entries that precede it, and that number is a bisection for its column in the same
// row of the other operand (the search of osp_apply_mask.h, in both directions).  Work is cut by entries in chunks of
// kCompactChunk, never by rows; a lane's kCompactRounds searches advance together.
//
// Union, hitsB(x) = the number of b's entries before position x whose coordinate is also in a (bit array + scan):
//   1. flag over b:   q' = lower bound of b.col[p'] in a's row (stored, u32), bit p' = a.col[q'] == b.col[p']
//   2. scan of the words' popcounts; the call's one read-back gives nnz_both
//   3. write b's side, a lane per entry: p' without its bit goes to p' + q' - hitsB(p')
//   4. write a's side, searching: p goes to p + q - hitsB(q), q = lower bound of a.col[p] in b's row; its value is
//      op(a[p], b[q]) when b.col[q] is its column
//   5. row pointer:   a.rowptr[i] + b.rowptr[i] - hitsB(b.rowptr[i])
// Intersect: flag over a (q stored), scan, compact_rowptr_kernel, and a write of op(a[p], b[q]) at the compacted position.
// Every output position is a function of bit arrays and searches alone: no atomics, nothing depends on processing order.
// The operator is a template parameter: there is no branch on it in a kernel.  Values that are only moved are moved as
// integers of their width.
#pragma once
#include "osp_compact.h"

namespace osp {

// (the values of osp_ewise_op_t)
enum { EW_PLUS = 0, EW_TIMES, EW_MIN, EW_MAX, EW_FIRST, EW_SECOND, EW_MINUS, EW_DIV, EW_OPS };

// the unsigned integer of a value's width
template <class T>
using ValueBits = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;

template <class T, class V>
__device__ __forceinline__ T ewise_as_value(V bits) {
    static_assert(sizeof(T) == sizeof(V), "a value and the integer of its width");
    T v;
    __builtin_memcpy(&v, &bits, sizeof v);
    return v;
}
template <class V, class T>
__device__ __forceinline__ V ewise_as_bits(T v) {
    static_assert(sizeof(T) == sizeof(V), "a value and the integer of its width");
    V bits;
    __builtin_memcpy(&bits, &v, sizeof bits);
    return bits;
}
// op(a, b) on the values' bits: ONE IEEE operation in T, or a copy of one operand's bits (MIN, MAX, FIRST, SECOND: the
// comparison is T's, what moves is the integer)
template <int OP, class T, class V>
__device__ __forceinline__ V ewise_apply(V a_bits, V b_bits) {
    const T a = ewise_as_value<T>(a_bits), b = ewise_as_value<T>(b_bits);
    switch (OP) {   // (OP is a constant: one case survives)
        case EW_PLUS: return ewise_as_bits<V>(a + b);
        case EW_TIMES: return ewise_as_bits<V>(a * b);
        case EW_MINUS: return ewise_as_bits<V>(a - b);
        case EW_DIV: return ewise_as_bits<V>(a / b);
        case EW_MIN: return b < a ? b_bits : a_bits;
        case EW_MAX: return b > a ? b_bits : a_bits;
        case EW_FIRST: return a_bits;
        default: return b_bits;   // EW_SECOND
    }
}

// entries before absolute position x (<= the flagged operand's nnz) whose bit is set
__device__ __forceinline__ uint64_t ewise_hits_before(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos, uint64_t x) {
    uint64_t h = pos[x >> 6];
    if (x & 63) h += (uint64_t)__popcll(bits[x >> 6] & ((1ull << (x & 63)) - 1ull));   // (x & 63 == 0: the word may not exist)
    return h;
}

// The lane's entries of x's chunk at `base` searched in y: p[k] the entry, j[k] its column, q[k] the absolute lower bound of
// j[k] in the same row of y (0 past the end), hit[k] whether y holds that coordinate.
// (positions in y and row numbers are kept in 32 bits: M and nnz(y) are below 2^32)
__device__ __forceinline__ void ewise_chunk_search(const int64_t *__restrict__ x_rowptr, const uint32_t *__restrict__ x_col, uint64_t M,
                                                   uint64_t nnz_x, uint64_t base, const int64_t *__restrict__ y_rowptr,
                                                   const uint32_t *__restrict__ y_col, int64_t (&p)[kCompactRounds],
                                                   uint32_t (&j)[kCompactRounds], uint32_t (&q)[kCompactRounds], bool (&hit)[kCompactRounds]) {
    uint32_t hi[kCompactRounds], end[kCompactRounds];
    chunk_entries_and_rows(x_rowptr, x_col, M, nnz_x, base, p, j, q, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint32_t r = q[k] - 1;
        const bool valid = (uint64_t)p[k] < nnz_x;
        q[k] = valid ? (uint32_t)y_rowptr[r] : 0u;
        hi[k] = valid ? (uint32_t)y_rowptr[r + 1] : 0u;
        end[k] = hi[k];
    }
    bisect_together<false>(y_col, q, hi, j);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) hit[k] = q[k] < end[k] && y_col[q[k]] == j[k];
}

// ---- pass 1 of both modes: one bit per entry of x (its coordinate is in y), and its lower bound in y ---------------------------
__global__ __launch_bounds__(kCompactThreads) void ewise_flag_kernel(const int64_t *__restrict__ x_rowptr, const uint32_t *__restrict__ x_col,
                                                                      uint64_t M, uint64_t nnz_x, const int64_t *__restrict__ y_rowptr,
                                                                      const uint32_t *__restrict__ y_col, uint64_t *__restrict__ bits,
                                                                      uint32_t *__restrict__ qpos) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_x) return;
    int64_t p[kCompactRounds];
    uint32_t j[kCompactRounds], q[kCompactRounds];
    bool hit[kCompactRounds];
    ewise_chunk_search(x_rowptr, x_col, M, nnz_x, base, y_rowptr, y_col, p, j, q, hit);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const bool valid = (uint64_t)p[k] < nnz_x;
        if (valid) qpos[p[k]] = q[k];
        store_verdicts(valid && hit[k], (uint64_t)p[k], nnz_x, bits);
    }
}

// ---- union, pass 3: b's entries that are not in a, a lane per entry, no search ----------------------------------------------------
template <class V>
__global__ __launch_bounds__(256) void ewise_union_write_b_kernel(const uint32_t *__restrict__ b_col, const V *__restrict__ b_val, uint64_t nnz_b,
                                                                  const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                                  const uint32_t *__restrict__ qpos, uint32_t *__restrict__ out_col,
                                                                  V *__restrict__ out_val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_b) return;
    const uint64_t word = bits[p >> 6];
    if ((word >> (p & 63)) & 1ull) return;   // a's side writes this coordinate
    const uint64_t o = p + (uint64_t)qpos[p] - (pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull)));
    out_col[o] = b_col[p];
    out_val[o] = b_val[p];
}

// ---- union, pass 4: every entry of a, searching b ------------------------------------------------------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(kCompactThreads) void ewise_union_write_a_kernel(
    const int64_t *__restrict__ a_rowptr, const uint32_t *__restrict__ a_col, const ValueBits<T> *__restrict__ a_val,
    uint64_t M, uint64_t nnz_a, const int64_t *__restrict__ b_rowptr, const uint32_t *__restrict__ b_col,
    const ValueBits<T> *__restrict__ b_val, const uint64_t *__restrict__ bits,
    const uint64_t *__restrict__ pos, uint32_t *__restrict__ out_col, ValueBits<T> *__restrict__ out_val) {
    typedef ValueBits<T> V;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz_a) return;
    int64_t p[kCompactRounds];
    uint32_t j[kCompactRounds], q[kCompactRounds];
    bool hit[kCompactRounds];
    ewise_chunk_search(a_rowptr, a_col, M, nnz_a, base, b_rowptr, b_col, p, j, q, hit);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if ((uint64_t)p[k] >= nnz_a) continue;
        const uint64_t o = (uint64_t)p[k] + (uint64_t)q[k] - ewise_hits_before(bits, pos, (uint64_t)q[k]);
        const V av = a_val[p[k]];
        out_col[o] = j[k];
        out_val[o] = hit[k] ? ewise_apply<OP, T, V>(av, b_val[q[k]]) : av;
    }
}

// ---- union, pass 5: out_rowptr[i] = a.rowptr[i] + b.rowptr[i] - hitsB(b.rowptr[i]), for i in [0, M] -------------------------------------
__global__ __launch_bounds__(256) void ewise_union_rowptr_kernel(const int64_t *__restrict__ a_rowptr, const int64_t *__restrict__ b_rowptr, uint64_t M,
                                                                 const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                                 int64_t *__restrict__ out_rowptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    const uint64_t pb = (uint64_t)b_rowptr[i];
    out_rowptr[i] = (int64_t)((uint64_t)a_rowptr[i] + pb - ewise_hits_before(bits, pos, pb));
}

// ---- intersect, pass 3: a's entries with their bit set, op(a[p], b[q]) at the compacted position -------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(256) void ewise_intersect_write_kernel(
    const uint32_t *__restrict__ a_col, const ValueBits<T> *__restrict__ a_val, uint64_t nnz_a,
    const ValueBits<T> *__restrict__ b_val, const uint64_t *__restrict__ bits,
    const uint64_t *__restrict__ pos, const uint32_t *__restrict__ qpos, uint32_t *__restrict__ out_col,
    ValueBits<T> *__restrict__ out_val) {
    typedef ValueBits<T> V;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz_a) return;
    const uint64_t word = bits[p >> 6];
    if ((word >> (p & 63)) & 1ull) {
        const uint64_t o = pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull));
        out_col[o] = a_col[p];
        // (FIRST reads no value of b, SECOND none of a: the unused load is gone with the constant OP)
        out_val[o] = ewise_apply<OP, T, V>(OP == EW_SECOND ? (V)0 : a_val[p], OP == EW_FIRST ? (V)0 : b_val[qpos[p]]);
    }
}

}  // namespace osp
