// osp_mxv.h -- a CSR result times a dense vector under a semiring (osp_csr_mxv, include/outerspace_spgemm_mxv.h), written
// for gfx950 (wave64).  DESIGN.md section 17.
//
// y[i] = R_add(mul(A[i, j_t], x[j_t])) with R the reduction of osp_vector.h, whose order depends on a row's length alone.
// The products are never written: a lane forms its product where wave_ordered_reduce would load a value, so the bits are
// those of osp_csr_apply_vectors followed by osp_csr_reduce.
//
// Packed rows.  With g a power of two, a wave takes 64 / g consecutive rows and gives each g lanes, when every row of the
// batch has at most g entries.  R of a row of m <= g entries by 64 lanes: lane l < m holds p_l = id (+) e_l, every other lane
// holds id, and the butterfly runs d = 32 .. 1.  A step d >= g combines p_l, l < d, with p_{l + d}, and l + d >= g >= m, so
// the right operand is id (or id (+) id, which is id) and the step changes no bit of p_l:
//   PLUS: p_l = +0.0 + e is never -0.0 (+0.0 + -0.0 is +0.0), so p_l + +0.0 is p_l (a NaN stays a NaN);
//   MIN:  +inf < p is false, p is kept; MAX: -inf > p is false, p is kept.
// What is left are the steps d = g/2 .. 1, and in them lane 0's value depends on the lanes below g alone: g lanes and
// log2(g) shuffles are the whole of R.  (__shfl_down reaches across a group's end only for lanes whose value nobody uses.)
// A batch with a row of more than g entries is found by a wave-uniform test of the row lengths; the wave then takes the
// batch's rows one after another with all 64 lanes -- wave_ordered_reduce's loop with the product in front -- and leaves a
// row of more than kReduceBlock entries to the block path.  g = 64 is one wave per row.  No pass classifies or sorts rows.
//
// Long rows.  mxv_blocks_kernel is reduce_blocks_kernel with the product in front: one wave per block of kReduceBlock
// writes partial[w]; (blkptr, partial) are then segments of plain values for reduce_segments.
//
// add and mul are template parameters (no branch on them in a kernel); x[j] is a plain gather; no LDS, no atomics.
#pragma once
#include "osp_vector.h"

namespace osp {

// mul(A's value at p, x[col[p]]) as a T: ONE IEEE operation or a copy (ewise_apply).  SECOND loads no value of A, FIRST
// neither the column nor x: the unused loads are gone with the constant MUL.
template <class T, int MUL>
__device__ __forceinline__ T mxv_product(const uint32_t *__restrict__ col, const T *__restrict__ vals, const T *__restrict__ x, uint64_t p) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    const V a = MUL == EW_SECOND ? (V)0 : ewise_as_bits<V>(vals[p]);
    const V b = MUL == EW_FIRST ? (V)0 : ewise_as_bits<V>(x[col[p]]);
    return ewise_as_value<T>(ewise_apply<MUL, T, V>(a, b));
}

// R of the products of the entries [b, b + m) by ONE wave, m <= kReduceBlock: wave_ordered_reduce on values never stored
template <class T, int ADD, int MUL>
__device__ __forceinline__ T mxv_wave_reduce(const uint32_t *__restrict__ col, const T *__restrict__ vals, const T *__restrict__ x, uint64_t b,
                                             uint64_t m) {
    T p = ordered_identity<ADD, T>();
    for (uint64_t i = lane_id(); i < m; i += kWave) p = ordered_combine<ADD>(p, mxv_product<T, MUL>(col, vals, x, b + i));
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) p = ordered_combine<ADD>(p, __shfl_down(p, d, kWave));
    return p;
}

// ---- rows of at most kReduceBlock entries: 64 >> lg consecutive rows per wave, g = 1 << lg lanes each when all of them fit --
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxv_rows_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                       const T *__restrict__ vals, const T *__restrict__ x, uint64_t M, uint32_t lg,
                                                                       T *__restrict__ y) {
    const uint32_t lane = lane_id(), g = 1u << lg;
    const uint64_t r0 = ((uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6)) << (6 - lg);   // the batch's first row
    if (r0 >= M) return;
    const uint64_t row = r0 + (lane >> lg);
    int64_t b = 0;
    uint64_t m = 0;
    if (row < M) {
        b = rowptr[row];
        m = (uint64_t)(rowptr[row + 1] - b);
    }
    if (!__any(m > g)) {
        const uint32_t k = lane & (g - 1);
        T p = ordered_identity<ADD, T>();
        if (k < m) p = ordered_combine<ADD>(p, mxv_product<T, MUL>(col, vals, x, (uint64_t)b + k));
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1)
            if ((uint32_t)d < g) p = ordered_combine<ADD>(p, __shfl_down(p, d, kWave));   // (g is the same in every lane)
        if (k == 0 && row < M) y[row] = p;
        return;
    }
    // a row of the batch does not fit its g lanes: the rows one after another, 64 lanes each
    for (uint32_t r = 0; r < (kWave >> lg) && r0 + r < M; r++) {
        const uint64_t rb = (uint64_t)__shfl((long long)b, (int)(r << lg), kWave), rm = (uint64_t)__shfl((long long)m, (int)(r << lg), kWave);
        if (rm > kReduceBlock) continue;   // (the block path writes it)
        const T p = mxv_wave_reduce<T, ADD, MUL>(col, vals, x, rb, rm);
        if (lane == 0) y[r0 + r] = p;
    }
}

// ---- rows of more than kReduceBlock entries, first level: partial[w] = R(the products of block w) -----------------------------
// (reduce_blocks_kernel's cut: block w belongs to the long row k with blkptr[k] <= w < blkptr[k + 1])
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxv_blocks_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                         const T *__restrict__ vals, const T *__restrict__ x,
                                                                         const uint32_t *__restrict__ long_rows, const int64_t *__restrict__ blkptr,
                                                                         uint64_t n_long, T *__restrict__ partial) {
    const uint64_t w = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (w >= (uint64_t)blkptr[n_long]) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t k = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;   // (same addresses in every lane)
    const uint32_t row = long_rows[k];
    const uint64_t b = (uint64_t)rowptr[row] + (w - (uint64_t)blkptr[k]) * kReduceBlock, e = (uint64_t)rowptr[row + 1];
    const T r = mxv_wave_reduce<T, ADD, MUL>(col, vals, x, b, e - b < kReduceBlock ? e - b : (uint64_t)kReduceBlock);
    if (lane_id() == 0) partial[w] = r;
}

}  // namespace osp
