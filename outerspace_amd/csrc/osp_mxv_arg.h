// osp_mxv_arg.h -- a CSR result times a dense vector under (MIN | MAX, mul), with the column of the winning product
// (osp_csr_mxv_arg, include/outerspace_spgemm_mxv_arg.h), written for gfx950 (wave64).  DESIGN.md section 25.
//
// The kernels ARE osp_csr_mxv's (osp_vector.h's skeleton on osp_mxv.h's Products) with another accumulator: the same row
// packing (64 >> lg rows per wave, the wave-uniform fall-back to 64 lanes per row), the same blocks of kReduceBlock for long
// rows, the same butterfly.  A lane carries (p, c), PairAcc below: p is mxv's partial, combined by ordered_combine exactly as
// there, so y keeps mxv's bits; c is the column of the best product the lane has seen, kArgNone (above any column:
// N <= 2^32 - 1) while it has seen none.
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
// Long rows: segments_blocks_kernel writes one (p, c) per block (Pairs); reduce_segments reduces those pairs per long row
// with the kernels and in the order of plain values (level by level where a row has more than kReduceBlock blocks), so the
// value side is osp_csr_mxv's to the bit.
//
// add and mul are template parameters; y is always formed (the host passes a pool buffer when the caller wants positions
// only: no branch on it here); no LDS, no atomics, no waiting between workgroups in the three paths.  arg_count_kernel, which
// counts the rows without a winner for the stats, is the one exception: a workgroup's scan and one integer atomic each.
#pragma once
#include "osp_mxv.h"

namespace osp {

constexpr uint32_t kArgNone = 0xffffffffu;   // the column of a pair that holds no product yet

__device__ __forceinline__ int64_t arg_of(uint32_t c) { return c == kArgNone ? (int64_t)-1 : (int64_t)c; }

// stored pairs: a source, and the sink of a level's partial pairs
template <class T>
struct Pairs {
    T *vals;
    uint32_t *cols;
    __device__ __forceinline__ uint32_t column(uint64_t i) const { return cols[i]; }
    __device__ __forceinline__ T value(uint64_t i, uint32_t = 0) const { return vals[i]; }
    template <class Acc>
    __device__ __forceinline__ void store(uint64_t i, const Acc &a) const {
        vals[i] = a.p;
        cols[i] = a.c;
    }
};

// the sink of the final pairs: the value and the position the caller sees
template <class T>
struct ArgSink {
    T *out;
    int64_t *arg;
    template <class Acc>
    __device__ __forceinline__ void store(uint64_t i, const Acc &a) const {
        out[i] = a.p;
        arg[i] = arg_of(a.c);
    }
};

template <int ADD, class T>
struct PairAcc {
    static_assert(ADD == RED_MIN || ADD == RED_MAX, "a position is defined for MIN and MAX");
    typedef Pairs<T> Stored;
    T p = ordered_identity<ADD, T>();
    uint32_t c = kArgNone;
    // (p, c) <- (p, c) (+) (q, d): c by the rule above on the OLD p, then p by mxv's combine
    __device__ __forceinline__ void combine(const PairAcc &o) {
        const bool better = ADD == RED_MIN ? o.p < p : o.p > p;
        if (better || (o.p == p && o.c < c)) c = o.c;
        p = ordered_combine<ADD>(p, o.p);
    }
    template <class Src>
    __device__ __forceinline__ void take(const Src &src, uint64_t i) {
        const uint32_t j = src.column(i);
        combine(PairAcc{src.value(i, j), j});
    }
    __device__ __forceinline__ PairAcc down(int d) const { return PairAcc{__shfl_down(p, d, kWave), (uint32_t)__shfl_down((int)c, d, kWave)}; }
};

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
