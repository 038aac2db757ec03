// osp_mxd.h -- a CSR result times a dense matrix under a semiring (osp_csr_mxd, include/outerspace_spgemm_mxd.h), written for
// gfx950 (wave64).  DESIGN.md section 21.
//
// y[i, c] = R_add(mul(A[i, j_t], x[j_t, c])): column c of y is osp_csr_mxv of column c of x, bit for bit.
//
// Layout.  A lane owns ONE (row, column) pair.  With kt = 1 << lgk the power of two >= min(k, 64), a wave holds 64 / kt
// consecutive rows and gives each kt lanes; for k > 64 blockIdx.y runs over column tiles of 64 (the last may be partial).  The
// lanes of a row read x[j, c0 .. c0 + kt): one coalesced row segment per entry; A's column and value at an entry are the same
// address in all of them.  Nothing crosses lanes: no shuffle, no LDS, no atomics.
//
// R by one lane.  R (osp_vector.h, osp_mxv.h) of m <= kReduceBlock values is a tree over w lane partials, w = 64 for m > 64
// and the power of two >= m otherwise (osp_mxv.h's header comment: the dropped lanes hold the identity and change no bit):
//   leaf  q_l    = id (+) e_l (+) e_{l + 64} (+) ...          (left to right)
//   node  V_d(l) = V_{2d}(l) (+) V_{2d}(l + d),   V_w(l) = q_l,   R = V_1(0).
// V_1(0)'s left subtree holds the even leaves, its right one the odd ones, and so on down: a depth-first walk meets the leaves
// in BIT-REVERSED order (0, 32, 16, 48, ... for w = 64).  The lane walks them in that order and keeps the finished subtrees
// like the digits of a binary counter: s[j] is a finished subtree of 2^j leaves.  After leaf number i, for every trailing
// 1-bit j of i, v = s[j] (+) v (the earlier subtree is the LEFT operand); at the first 0-bit, s[j] = v.  The last leaf has
// all bits set and leaves R in v.  j is a compile-time index (the loop over it is unrolled), so s[] lives in six registers:
// no scratch.  Every entry is read once.
//
// Long rows are listed and cut as mxv_impl lists and cuts them.  mxd_blocks_kernel gives each (block, column) to a lane --
// partial[w, c] = R(the products of block w in column c) -- and mxd_upper_kernel each (long row, column): the same function on
// the row's partials, and on blocks of kReduceBlock partials first when the row has more than kReduceBlock blocks (rows have
// fewer than 2^32 entries: at most 2^21 partials, 2^10 blocks of them, so two levels are all of R's recursion).
//
// add and mul are template parameters (no branch on them in a kernel).
#pragma once
#include "osp_mxv.h"

namespace osp {

constexpr uint32_t kMxdMaxCols = 65536;   // the largest k (OSP_MXD_MAX_COLS): the column tiles fit gridDim.y

// mul(A's value at p, x[col[p], c]) as a T: osp_mxv.h's Products::value with a row of x where it has one value
template <class T, int MUL>
__device__ __forceinline__ T mxd_product(const uint32_t *__restrict__ col, const T *__restrict__ vals, const T *__restrict__ x, uint64_t p,
                                         uint64_t k, uint64_t c) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    const V a = MUL == EW_SECOND ? (V)0 : ewise_as_bits<V>(vals[p]);
    const V b = MUL == EW_FIRST ? (V)0 : ewise_as_bits<V>(x[(uint64_t)col[p] * k + c]);
    return ewise_as_value<T>(ewise_apply<MUL, T, V>(a, b));
}

// R of entry(0) .. entry(m - 1), m <= kReduceBlock, by ONE lane in R's own operand order (the header comment)
template <class T, int ADD, class Entry>
__device__ __forceinline__ T mxd_serial_reduce(uint32_t m, Entry &&entry) {
    const uint32_t lgw = m > 32 ? 6u : m <= 1 ? 0u : 32u - (uint32_t)__clz((int)(m - 1));   // log2 of the leaves
    const T id = ordered_identity<ADD, T>();
    T s[6] = {id, id, id, id, id, id};
    T v = id;
    for (uint32_t i = 0; i < (1u << lgw); i++) {
        const uint32_t l = (__brev(i) >> 1) >> (31 - lgw);   // (lgw may be 0: no shift by 32)
        v = id;
        for (uint32_t t = l; t < m; t += kWave) v = ordered_combine<ADD>(v, entry(t));
#pragma unroll
        for (int j = 0; j < 6; j++) {
            if (!((i >> j) & 1u)) {
                s[j] = v;
                break;
            }
            v = ordered_combine<ADD>(s[j], v);
        }
    }
    return v;
}

// the (item, column) pair of this lane: 64 >> lgk consecutive items per wave, 1 << lgk lanes each; false: no pair
__device__ __forceinline__ bool mxd_lane_pair(uint32_t lgk, uint64_t nitems, uint64_t k, uint64_t &item, uint64_t &c) {
    const uint32_t lane = lane_id();
    item = (((uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6)) << (6 - lgk)) + (lane >> lgk);
    c = (uint64_t)blockIdx.y * kWave + (lane & ((1u << lgk) - 1));
    return item < nitems && c < k;
}

// ---- rows of at most kReduceBlock entries ---------------------------------------------------------------------------------------
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxd_rows_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                       const T *__restrict__ vals, const T *__restrict__ x, uint64_t M, uint64_t k,
                                                                       uint32_t lgk, T *__restrict__ y) {
    uint64_t row, c;
    if (!mxd_lane_pair(lgk, M, k, row, c)) return;
    const uint64_t b = (uint64_t)rowptr[row], m = (uint64_t)rowptr[row + 1] - b;
    if (m > kReduceBlock) return;   // (the block path writes it)
    y[row * k + c] = mxd_serial_reduce<T, ADD>((uint32_t)m, [&](uint32_t t) { return mxd_product<T, MUL>(col, vals, x, b + t, k, c); });
}

// ---- rows of more than kReduceBlock entries, first level: partial[w, c] = R(the products of block w in column c) -----------------
// (segments_blocks_kernel's cut: block w belongs to the long row r with blkptr[r] <= w < blkptr[r + 1])
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxd_blocks_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                         const T *__restrict__ vals, const T *__restrict__ x,
                                                                         const uint32_t *__restrict__ long_rows, const int64_t *__restrict__ blkptr,
                                                                         uint64_t n_long, uint64_t k, uint32_t lgk, T *__restrict__ partial) {
    uint64_t w, c;
    if (!mxd_lane_pair(lgk, (uint64_t)blkptr[n_long], k, w, c)) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t r = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;
    const uint32_t row = long_rows[r];
    const uint64_t b = (uint64_t)rowptr[row] + (w - (uint64_t)blkptr[r]) * kReduceBlock, e = (uint64_t)rowptr[row + 1];
    const uint32_t m = e - b < kReduceBlock ? (uint32_t)(e - b) : kReduceBlock;
    partial[w * k + c] = mxd_serial_reduce<T, ADD>(m, [&](uint32_t t) { return mxd_product<T, MUL>(col, vals, x, b + t, k, c); });
}

// ---- the upper levels: y[long row r, c] = R(partial[blkptr[r] .. blkptr[r + 1], c]) -----------------------------------------------
template <class T, int ADD>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxd_upper_kernel(const uint32_t *__restrict__ long_rows, const int64_t *__restrict__ blkptr,
                                                                        uint64_t n_long, const T *__restrict__ partial, uint64_t k, uint32_t lgk,
                                                                        T *__restrict__ y) {
    uint64_t r, c;
    if (!mxd_lane_pair(lgk, n_long, k, r, c)) return;
    const uint64_t first = (uint64_t)blkptr[r], nb = (uint64_t)blkptr[r + 1] - first;
    const T *__restrict__ p = partial + first * k + c;
    T v;
    if (nb <= kReduceBlock) {
        v = mxd_serial_reduce<T, ADD>((uint32_t)nb, [&](uint32_t t) { return p[(uint64_t)t * k]; });
    } else {   // the partials are a long segment themselves: R of its blocks, then R of those
        v = mxd_serial_reduce<T, ADD>((uint32_t)((nb + kReduceBlock - 1) / kReduceBlock), [&](uint32_t t2) {
            const uint64_t o = (uint64_t)t2 * kReduceBlock;
            return mxd_serial_reduce<T, ADD>(nb - o < kReduceBlock ? (uint32_t)(nb - o) : kReduceBlock, [&](uint32_t t) { return p[(o + t) * k]; });
        });
    }
    y[(uint64_t)long_rows[r] * k + c] = v;
}

}  // namespace osp
