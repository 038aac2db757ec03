// osp_mxv_arg.h -- a CSR result times a dense vector under (MIN | MAX, mul), with the column of the winning product
// (osp_csr_mxv_arg, include/outerspace_spgemm_mxv_arg.h), written for gfx950 (wave64).  DESIGN.md section 25.
//
// The kernels are osp_mxv.h's with a column beside the lane's partial: the same row packing (64 >> lg rows per wave, the
// wave-uniform fall-back to 64 lanes per row), the same blocks of kReduceBlock for long rows, the same butterfly.  A lane
// carries (p, c): p is mxv's partial, combined by ordered_combine exactly as there, so y keeps mxv's bits; c is the column of
// the best product the lane has seen, kArgNone (above any column: N <= 2^32 - 1) while it has seen none.
//
// The pair's value IS p.  p starts as the identity and ordered_combine keeps it over a NaN, so p is always the smallest
// (MIN) or largest (MAX) non-NaN product seen so far as a NUMBER; only the sign of a zero depends on the order.  The rule
// that moves c compares numbers alone (-0.0 == +0.0), so a separate "best value" would be a second copy of p:
//   (q, d) enters (p, c) when q is better than p, or q == p and d < c.
// A NaN q is neither better nor equal: it never enters.  A product equal to the identity enters over kArgNone (d < kArgNone),
// so a row whose only non-NaN product is +inf under MIN reports that product's column, and c == kArgNone says "nothing".
// (number, column) under "better number, then smaller column" is a total preorder and the rule is its minimum, which is
// associative and commutative: c depends neither on the reduction tree, nor on g, nor on where a long row is cut.
//
// Long rows: mxv_arg_blocks_kernel writes one (p, c) per block; arg_short_kernel / arg_blocks_kernel reduce those pairs per
// long row in reduce_short_kernel's / reduce_blocks_kernel's order (level by level where a row has more than kReduceBlock
// blocks), so the value side is reduce_segments' to the bit.
//
// add and mul are template parameters; y is always formed (the host passes a pool buffer when the caller wants positions
// only: no branch on it here); no LDS, no atomics, no waiting between workgroups in the three paths.  arg_count_kernel, which
// counts the rows without a winner for the stats, is the one exception: a workgroup's scan and one integer atomic each.
#pragma once
#include "osp_mxv.h"

namespace osp {

constexpr uint32_t kArgNone = 0xffffffffu;   // the column of a pair that holds no product yet

// (p, c) <- (p, c) (+) (q, d): c by the rule above on the OLD p, then p by mxv's combine
template <int ADD, class T>
__device__ __forceinline__ void arg_combine(T &p, uint32_t &c, T q, uint32_t d) {
    static_assert(ADD == RED_MIN || ADD == RED_MAX, "a position is defined for MIN and MAX");
    const bool better = ADD == RED_MIN ? q < p : q > p;
    if (better || (q == p && d < c)) c = d;
    p = ordered_combine<ADD>(p, q);
}

// the butterfly's steps d < below on pairs (below = 64: a whole wave; below = g: a packed row's g lanes)
template <int ADD, class T>
__device__ __forceinline__ void arg_butterfly(T &p, uint32_t &c, uint32_t below) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1)
        if ((uint32_t)d < below) {   // (below is the same in every lane)
            const T q = __shfl_down(p, d, kWave);
            const uint32_t e = (uint32_t)__shfl_down((int)c, d, kWave);
            arg_combine<ADD>(p, c, q, e);
        }
}

// mul(A's value at q, x[j]) with j = col[q], which the caller needs as well.  SECOND loads no value of A, FIRST no x.
template <class T, int MUL>
__device__ __forceinline__ T mxv_arg_product(const uint32_t *__restrict__ col, const T *__restrict__ vals, const T *__restrict__ x, uint64_t q,
                                             uint32_t &j) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    j = col[q];
    const V a = MUL == EW_SECOND ? (V)0 : ewise_as_bits<V>(vals[q]);
    const V b = MUL == EW_FIRST ? (V)0 : ewise_as_bits<V>(x[j]);
    return ewise_as_value<T>(ewise_apply<MUL, T, V>(a, b));
}

// mxv_wave_reduce with the column: R of the products of the entries [b, b + m) by ONE wave, m <= kReduceBlock
template <class T, int ADD, int MUL>
__device__ __forceinline__ T mxv_arg_wave_reduce(const uint32_t *__restrict__ col, const T *__restrict__ vals, const T *__restrict__ x, uint64_t b,
                                                 uint64_t m, uint32_t &c) {
    T p = ordered_identity<ADD, T>();
    c = kArgNone;
    for (uint64_t i = lane_id(); i < m; i += kWave) {
        uint32_t j;
        const T q = mxv_arg_product<T, MUL>(col, vals, x, b + i, j);
        arg_combine<ADD>(p, c, q, j);
    }
    arg_butterfly<ADD>(p, c, kWave);
    return p;
}

__device__ __forceinline__ int64_t arg_of(uint32_t c) { return c == kArgNone ? (int64_t)-1 : (int64_t)c; }

// ---- rows of at most kReduceBlock entries: mxv_rows_kernel on pairs -------------------------------------------------------------
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxv_arg_rows_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                           const T *__restrict__ vals, const T *__restrict__ x, uint64_t M, uint32_t lg,
                                                                           T *__restrict__ y, int64_t *__restrict__ arg) {
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
        uint32_t c = kArgNone;
        if (k < m) {
            uint32_t j;
            const T q = mxv_arg_product<T, MUL>(col, vals, x, (uint64_t)b + k, j);
            arg_combine<ADD>(p, c, q, j);
        }
        // (a lane past its row's entries holds (identity, kArgNone), which changes no pair it is combined into; a shuffle
        // reaches across a group's end only for lanes whose pair nobody uses: osp_mxv.h)
        arg_butterfly<ADD>(p, c, g);
        if (k == 0 && row < M) {
            y[row] = p;
            arg[row] = arg_of(c);
        }
        return;
    }
    // a row of the batch does not fit its g lanes: the rows one after another, 64 lanes each
    for (uint32_t r = 0; r < (kWave >> lg) && r0 + r < M; r++) {
        const uint64_t rb = (uint64_t)__shfl((long long)b, (int)(r << lg), kWave), rm = (uint64_t)__shfl((long long)m, (int)(r << lg), kWave);
        if (rm > kReduceBlock) continue;   // (the block path writes it)
        uint32_t c;
        const T p = mxv_arg_wave_reduce<T, ADD, MUL>(col, vals, x, rb, rm, c);
        if (lane == 0) {
            y[r0 + r] = p;
            arg[r0 + r] = arg_of(c);
        }
    }
}

// ---- rows of more than kReduceBlock entries, first level: (partial[w], pcol[w]) = the pair of block w -------------------------------
// (mxv_blocks_kernel's cut)
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void mxv_arg_blocks_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                             const T *__restrict__ vals, const T *__restrict__ x,
                                                                             const uint32_t *__restrict__ long_rows, const int64_t *__restrict__ blkptr,
                                                                             uint64_t n_long, T *__restrict__ partial, uint32_t *__restrict__ pcol) {
    const uint64_t w = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (w >= (uint64_t)blkptr[n_long]) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t k = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;   // (same addresses in every lane)
    const uint32_t row = long_rows[k];
    const uint64_t b = (uint64_t)rowptr[row] + (w - (uint64_t)blkptr[k]) * kReduceBlock, e = (uint64_t)rowptr[row + 1];
    uint32_t c;
    const T r = mxv_arg_wave_reduce<T, ADD, MUL>(col, vals, x, b, e - b < kReduceBlock ? e - b : (uint64_t)kReduceBlock, c);
    if (lane_id() == 0) {
        partial[w] = r;
        pcol[w] = c;
    }
}

// ---- the second level: segments of pairs --------------------------------------------------------------------------------------------
// wave_ordered_reduce on the pairs (vals[i], cols[i]), i in [0, m)
template <int ADD, class T>
__device__ __forceinline__ T arg_wave_reduce(const T *__restrict__ vals, const uint32_t *__restrict__ cols, uint64_t m, uint32_t &c) {
    T p = ordered_identity<ADD, T>();
    c = kArgNone;
    for (uint64_t i = lane_id(); i < m; i += kWave) arg_combine<ADD>(p, c, vals[i], cols[i]);
    arg_butterfly<ADD>(p, c, kWave);
    return p;
}

// reduce_short_kernel on pairs: (out, arg)[map[seg]] = the pair of segment seg; longer segments are left to the block path
template <class T, int ADD>
__global__ __launch_bounds__(kReduceWaves *kWave) void arg_short_kernel(const int64_t *__restrict__ ptr, const T *__restrict__ vals,
                                                                        const uint32_t *__restrict__ cols, uint64_t nseg,
                                                                        const uint32_t *__restrict__ map, T *__restrict__ out, int64_t *__restrict__ arg) {
    const uint64_t seg = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const int64_t b = ptr[seg];
    const uint64_t m = (uint64_t)(ptr[seg + 1] - b);
    if (m > kReduceBlock) return;
    uint32_t c;
    const T r = arg_wave_reduce<ADD>(vals + b, cols + b, m, c);
    if (lane_id() == 0) {
        out[map[seg]] = r;
        arg[map[seg]] = arg_of(c);
    }
}

// reduce_blocks_kernel on pairs: (partial[w], pcol[w]) = the pair of block w of the long segments
template <class T, int ADD>
__global__ __launch_bounds__(kReduceWaves *kWave) void arg_blocks_kernel(const int64_t *__restrict__ ptr, const T *__restrict__ vals,
                                                                         const uint32_t *__restrict__ cols, const uint32_t *__restrict__ long_segs,
                                                                         const int64_t *__restrict__ blkptr, uint64_t n_long, T *__restrict__ partial,
                                                                         uint32_t *__restrict__ pcol) {
    const uint64_t w = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (w >= (uint64_t)blkptr[n_long]) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t k = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;   // (same addresses in every lane)
    const uint32_t seg = long_segs[k];
    const uint64_t b = (uint64_t)ptr[seg] + (w - (uint64_t)blkptr[k]) * kReduceBlock, e = (uint64_t)ptr[seg + 1];
    uint32_t c;
    const T r = arg_wave_reduce<ADD>(vals + b, cols + b, e - b < kReduceBlock ? e - b : (uint64_t)kReduceBlock, c);
    if (lane_id() == 0) {
        partial[w] = r;
        pcol[w] = c;
    }
}

// ---- the stats' rows_without: *out += the rows with arg == -1 (few workgroups, one atomic each) ------------------------------------
__global__ __launch_bounds__(256) void arg_count_kernel(const int64_t *__restrict__ arg, uint64_t M, unsigned long long *__restrict__ out) {
    __shared__ uint64_t scratch[256 / kWave + 1];
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (uint64_t)gridDim.x * blockDim.x) sum += arg[i] < 0;
    uint64_t total;
    block_excl_scan<uint64_t, 256>(sum, scratch, &total);
    if (threadIdx.x == 0 && total) atomicAdd(out, (unsigned long long)total);
}

}  // namespace osp
