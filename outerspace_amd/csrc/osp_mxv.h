// osp_mxv.h -- a CSR result times a dense vector under a semiring (osp_csr_mxv, include/outerspace_spgemm_mxv.h), written
// for gfx950 (wave64).  DESIGN.md section 17.
//
// y[i] = R_add(mul(A[i, j_t], x[j_t])) with R the reduction of osp_vector.h, whose order depends on a row's length alone.
// The products are never written: they are a SOURCE of osp_vector.h's skeleton (Products below), so a lane forms its product
// where osp_csr_reduce loads a value and the bits are those of osp_csr_apply_vectors followed by osp_csr_reduce.
//
// Packed rows (segments_rows_kernel, osp_vector.h).  With g a power of two, a wave takes 64 / g consecutive rows and gives
// each g lanes, when every row of the batch has at most g entries.  R of a row of m <= g entries by 64 lanes: lane l < m holds p_l = id (+) e_l, every other lane
// holds id, and the butterfly runs d = 32 .. 1.  A step d >= g combines p_l, l < d, with p_{l + d}, and l + d >= g >= m, so
// the right operand is id (or id (+) id, which is id) and the step changes no bit of p_l:
//   PLUS: p_l = +0.0 + e is never -0.0 (+0.0 + -0.0 is +0.0), so p_l + +0.0 is p_l (a NaN stays a NaN);
//   MIN:  +inf < p is false, p is kept; MAX: -inf > p is false, p is kept.
// What is left are the steps d = g/2 .. 1, and in them lane 0's value depends on the lanes below g alone: g lanes and
// log2(g) shuffles are the whole of R.  (__shfl_down reaches across a group's end only for lanes whose value nobody uses.)
// A batch with a row of more than g entries is found by a wave-uniform test of the row lengths; the wave then takes the
// batch's rows one after another with all 64 lanes -- wave_reduce on the products -- and leaves a row of more than
// kReduceBlock entries to the block path.  g = 64 is one wave per row.  No pass classifies or sorts rows.
//
// Long rows.  segments_blocks_kernel on the products: one wave per block of kReduceBlock writes partial[w]; (blkptr, partial)
// are then segments of plain values for reduce_segments.
//
// add and mul are template parameters (no branch on them in a kernel); x[j] is a plain gather; no LDS, no atomics.
#pragma once
#include "osp_vector.h"

namespace osp {

// the products of A's entries with x as a source: value(i) = mul(A's value at i, x[col[i]]) as a T, ONE IEEE operation or a copy
// (ewise_apply).  SECOND loads no value of A, FIRST no x -- and no column either where the accumulator asks for none
// (PlainAcc): the unused loads are gone with the constant MUL.  A PairAcc loads the column once and passes it back.
template <class T, int MUL>
struct Products {
    const uint32_t *col;
    const T *vals, *x;
    __device__ __forceinline__ uint32_t column(uint64_t i) const { return col[i]; }
    __device__ __forceinline__ T value(uint64_t i, uint32_t j) const {
#pragma clang fp contract(off)
        typedef ValueBits<T> V;
        const V a = MUL == EW_SECOND ? (V)0 : ewise_as_bits<V>(vals[i]);
        const V b = MUL == EW_FIRST ? (V)0 : ewise_as_bits<V>(x[j]);
        return ewise_as_value<T>(ewise_apply<MUL, T, V>(a, b));
    }
    __device__ __forceinline__ T value(uint64_t i) const { return value(i, MUL == EW_FIRST ? 0u : col[i]); }
};

}  // namespace osp
