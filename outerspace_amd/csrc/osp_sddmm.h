// osp_sddmm.h -- the sampled dense-dense product on a CSR result's pattern under a semiring (osp_csr_sddmm,
// include/outerspace_spgemm_sddmm.h), written for gfx950 (wave64).  DESIGN.md section 23.
//
// out(i, j) = accum(in(i, j), d),  d = R_add(p_0 .. p_{k-1}),  p_c = mul(x[i, c], y[j, c]),  for the entries (i, j) of `in`.
// d is osp_csr_mxv of the one-row CSR that holds x[i, 0..k) at the columns 0..k-1 with the vector y[j, :], bit for bit.
//
// Work is cut by ENTRIES.  A wave owns 64 consecutive entries of `in`, whatever rows they lie in: lane e loads the column of
// entry p0 + e (one coalesced load) and finds its row by a bisection of rowptr between the rows of the wave's first and last
// entry (no trip when the 64 entries lie in one row; an empty row is an index the bisection steps over; a row of 4097 entries
// is 65 waves like any other 4097 entries).  The (row, column) pairs then travel by __shfl as the wave needs them.
//
// Lanes across k.  With kt = 1 << lgk the power of two >= min(k, 64), the wave takes its entries in batches of 64 / kt and
// gives each kt lanes.  Lane l of a group reads x[i, l + kt t] and y[j, l + kt t], t = 0, 1, ...: coalesced row segments.
//   * k <= 64: a lane holds one product at most.  R of k <= kt values by 64 lanes is lane l < k holding id (+) p_l, every
//     other lane the identity, and the butterfly d = 32 .. 1; the steps d >= kt change no bit (osp_mxv.h's header comment), so
//     the group's steps d = kt/2 .. 1 are all of R.  (__shfl_down reaches across a group's end only for lanes whose value
//     nobody uses.)
//   * 64 < k <= kReduceBlock: kt = 64, a lane folds its products left to right with stride 64 into the identity, then the
//     butterfly: wave_ordered_reduce with the product in front.
//   * k > kReduceBlock: R is R over the R of the blocks of kReduceBlock.  The wave walks the nb = ceil(k / kReduceBlock) <= 32
//     blocks (k <= kMxdMaxCols), lane b keeps id (+) r_b, lanes >= nb the identity, and one more butterfly gives R of those:
//     two levels are all of the recursion.
// Lane 0 of a group applies accum -- a wave-uniform runtime switch over ewise_apply's operators, `in`'s value in a's place --
// and stores.  SECOND loads no value of `in`.
//
// add and mul are template parameters (no branch on them in a kernel).  No LDS, no atomics, no waiting between workgroups.
#pragma once
#include "osp_mxd.h"

namespace osp {

// mul(x[i, c], y[j, c]) as a T: ONE IEEE operation or a copy (ewise_apply).  FIRST loads no y, SECOND no x.
template <class T, int MUL>
__device__ __forceinline__ T sddmm_product(const T *__restrict__ x, const T *__restrict__ y, uint64_t xi, uint64_t yj, uint64_t c) {
#pragma clang fp contract(off)
    typedef ValueBits<T> V;
    const V a = MUL == EW_SECOND ? (V)0 : ewise_as_bits<V>(x[xi + c]);
    const V b = MUL == EW_FIRST ? (V)0 : ewise_as_bits<V>(y[yj + c]);
    return ewise_as_value<T>(ewise_apply<MUL, T, V>(a, b));
}

// accum(c, d) in osp_csr_apply_vectors' operator table; SECOND (and everything outside the table) is d's bits
template <class T>
__device__ __forceinline__ ValueBits<T> sddmm_accum(int accum, ValueBits<T> c, ValueBits<T> d) {
    typedef ValueBits<T> V;
    switch (accum) {
        case EW_PLUS: return ewise_apply<EW_PLUS, T, V>(c, d);
        case EW_TIMES: return ewise_apply<EW_TIMES, T, V>(c, d);
        case EW_MINUS: return ewise_apply<EW_MINUS, T, V>(c, d);
        case EW_DIV: return ewise_apply<EW_DIV, T, V>(c, d);
        case EW_MIN: return ewise_apply<EW_MIN, T, V>(c, d);
        case EW_MAX: return ewise_apply<EW_MAX, T, V>(c, d);
        default: return d;
    }
}

// (the grid covers ceil(nnz / 64) waves; nnz > 0, so N >= 1 and M >= 1)
template <class T, int ADD, int MUL>
__global__ __launch_bounds__(kReduceWaves *kWave) void sddmm_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                    const ValueBits<T> *__restrict__ in_vals, const T *__restrict__ x,
                                                                    const T *__restrict__ y, uint64_t M, uint64_t nnz, uint64_t k, uint32_t lgk,
                                                                    int accum, ValueBits<T> *__restrict__ out_vals) {
    typedef ValueBits<T> V;
    const uint32_t lane = lane_id();
    const uint64_t p0 = ((uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6)) * kWave;   // the wave's first entry
    if (p0 >= nnz) return;
    const uint64_t last = (p0 + kWave < nnz ? p0 + kWave : nnz) - 1;
    // the rows of the wave's first and last entry (the last row r with rowptr[r] <= p holds entry p; same addresses in every
    // lane), then this lane's entry between them
    const uint32_t r_first = (uint32_t)(upper_bound_dev(rowptr, 0, M + 1, (int64_t)p0) - 1);
    const uint32_t r_last = (uint32_t)(upper_bound_dev(rowptr, (uint64_t)r_first + 1, M + 1, (int64_t)last) - 1);
    const uint64_t mine = p0 + lane;
    const uint32_t my_col = mine < nnz ? col[mine] : 0u;
    uint32_t my_row = r_first;
    if (r_first != r_last && mine < nnz) my_row = (uint32_t)(upper_bound_dev(rowptr, (uint64_t)r_first + 1, (uint64_t)r_last + 1, (int64_t)mine) - 1);

    const uint32_t per = kWave >> lgk, l = lane & ((1u << lgk) - 1u);   // entries per batch, this lane's place in its group
    const T id = ordered_identity<ADD, T>();
    for (uint32_t first = 0; first < kWave && p0 + first < nnz; first += per) {
        const uint32_t e = first + (lane >> lgk);   // this group's entry of the wave
        const bool live = p0 + e < nnz;             // (past the end: row r_first, column 0; nothing is loaded for it)
        const uint64_t xi = (uint64_t)(uint32_t)__shfl((int)my_row, (int)e, kWave) * k;   // where x[i, :] and y[j, :] begin
        const uint64_t yj = (uint64_t)(uint32_t)__shfl((int)my_col, (int)e, kWave) * k;
        T d = id;
        if (k <= kReduceBlock) {
            if (live)
                for (uint64_t c = l; c < k; c += (uint64_t)1 << lgk) d = ordered_combine<ADD>(d, sddmm_product<T, MUL>(x, y, xi, yj, c));
#pragma unroll
            for (int s = kWave / 2; s > 0; s >>= 1)
                if ((uint32_t)s < (1u << lgk)) d = ordered_combine<ADD>(d, __shfl_down(d, s, kWave));   // (lgk is the same in every lane)
        } else {   // (lgk == 6: the wave holds one entry)
            for (uint64_t c0 = 0, b = 0; c0 < k; c0 += kReduceBlock, b++) {
                const uint64_t c1 = c0 + kReduceBlock < k ? c0 + kReduceBlock : k;
                T r = id;
                for (uint64_t c = c0 + lane; c < c1; c += kWave) r = ordered_combine<ADD>(r, sddmm_product<T, MUL>(x, y, xi, yj, c));
#pragma unroll
                for (int s = kWave / 2; s > 0; s >>= 1) r = ordered_combine<ADD>(r, __shfl_down(r, s, kWave));
                r = __shfl(r, 0, kWave);
                if (lane == b) d = ordered_combine<ADD>(d, r);
            }
#pragma unroll
            for (int s = kWave / 2; s > 0; s >>= 1) d = ordered_combine<ADD>(d, __shfl_down(d, s, kWave));
        }
        if (l == 0 && live) {
            const bool reads = accum >= EW_PLUS && accum != EW_FIRST && accum != EW_SECOND && accum <= EW_DIV;
            out_vals[p0 + e] = sddmm_accum<T>(accum, reads ? in_vals[p0 + e] : (V)0, ewise_as_bits<V>(d));
        }
    }
}

}  // namespace osp
