// osp_mcl.h -- one step of Markov clustering between two expansions (osp_csr_inflate_prune,
// include/outerspace_spgemm_mcl.h), written for gfx950 (wave64).  DESIGN.md section 10.
//
// Per row of a CSR result: prune (threshold, rescue, keep the k largest), inflate, normalise, chaos.  Two passes around the
// library's exclusive scan, as osp_csr_bias_relu:
//   1. count: one read of the values; a row's kept count follows from its survivor count alone (min(survivors, cap), or 1
//      when nothing survives), so no selection is needed to size the output;
//   2. write: a row whose candidates all stay is streamed once; a row that loses entries to the cap (or is rescued) first
//      finds the value of its k-th largest candidate by a radix select on the value's bit pattern, 8 bits a pass from the
//      top, stopping as soon as the bucket that holds the k-th value is taken whole; then the row is streamed once more and
//      the kept entries are compacted in column order (ties by a prefix count in row order), inflated, summed and divided.
// Rows up to kMclLongMin entries are handled by one wave each, longer ones by one workgroup of 256 threads each: the same
// code with NT = 64 or 256 (one row per workgroup, so __syncthreads is the only synchronisation in both).
//
// Non-negative IEEE values order like their bit patterns read as unsigned integers, so the select needs no key transform
// (-0.0 is given the key of +0.0).  Sums: every lane l adds the kept entries l, l + 64, ... left to right, then a butterfly
// over the 64 partial sums -- ONE wave per row forms them whatever the row's class, so the order depends on the row's kept
// values alone.  No product is contracted into an addition (`#pragma clang fp contract(off)`).
#pragma once
#include <type_traits>

#include "osp_prims.h"

namespace osp {

// rows with more entries than this take the one-workgroup-per-row path (OSP_MCL_LONG_MIN overrides it for measurement)
constexpr uint32_t kMclLongMin = 2048;
constexpr int kMclLongThreads = 256;
// device counters of one call
enum { MCL_CAPPED = 0, MCL_RESCUED = 1, MCL_CHAOS = 2, MCL_INVALID = 3, MCL_NLONG = 4, MCL_COUNTERS = 5 };
enum { MCL_POW_ONE = 0, MCL_POW_SQUARE = 1, MCL_POW_GENERAL = 2 };

template <class T> struct MclKey;
template <> struct MclKey<float> { typedef uint32_t type; };
template <> struct MclKey<double> { typedef uint64_t type; };

template <class T>
__device__ __forceinline__ typename MclKey<T>::type mcl_key(T v) {
    typedef typename MclKey<T>::type K;
    if (v == T(0)) return K(0);   // (-0.0 orders as +0.0)
    K k;
    __builtin_memcpy(&k, &v, sizeof(K));
    return k;
}
template <class T>
__device__ __forceinline__ T mcl_inflate(T v, int mode, T power) {
#pragma clang fp contract(off)
    if (mode == MCL_POW_ONE) return v;
    if (mode == MCL_POW_SQUARE) return v * v;
    if constexpr (std::is_same<T, float>::value) return powf(v, power);
    else return pow(v, power);
}

// flag = 1 when a value is negative, NaN or infinite
template <class T>
__global__ __launch_bounds__(256) void mcl_validate_kernel(const T *__restrict__ val, uint64_t nnz, unsigned long long *__restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = i < nnz && !(val[i] >= T(0) && val[i] < (T)__builtin_inf());
    if (__ballot(bad) && lane_id() == 0) atomicOr(&counters[MCL_INVALID], 1ull);
}

// the rows longer than long_min, in any order (every row is handled on its own, so the order does not reach the result)
__global__ __launch_bounds__(256) void mcl_classify_kernel(const int64_t *__restrict__ rowptr, uint64_t M, uint32_t long_min,
                                                           uint32_t *__restrict__ long_rows, unsigned long long *__restrict__ counters) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    if ((uint64_t)(rowptr[r + 1] - rowptr[r]) > long_min) long_rows[atomicAdd(&counters[MCL_NLONG], 1ull)] = (uint32_t)r;
}

// The row of workgroup `blockIdx.x`: row0 + blockIdx.x of the short class (rows of the long class return at once), or
// long_rows[blockIdx.x].
template <int NT>
__device__ __forceinline__ bool mcl_my_row(const int64_t *rowptr, uint64_t row0, uint64_t M, const uint32_t *long_rows, uint32_t long_min,
                                           uint64_t &r, int64_t &b, uint64_t &n) {
    if (NT == kWave) {
        r = row0 + blockIdx.x;
        if (r >= M) return false;
    } else {
        r = long_rows[blockIdx.x];
    }
    b = rowptr[r];
    n = (uint64_t)(rowptr[r + 1] - b);
    return NT == kWave ? n <= long_min : true;
}

// ---- pass 1: survivors and kept entries per row -------------------------------------------------------------------------
template <class T, int NT>
__global__ __launch_bounds__(NT) void mcl_count_kernel(const int64_t *__restrict__ rowptr, const T *__restrict__ val, uint64_t row0, uint64_t M,
                                                       const uint32_t *__restrict__ long_rows, uint32_t long_min, T thr, uint32_t cap,
                                                       uint32_t *__restrict__ nsurv, uint32_t *__restrict__ cnt,
                                                       unsigned long long *__restrict__ counters) {
    constexpr int NW = NT / kWave;
    __shared__ uint32_t part[NW];
    uint64_t r, n;
    int64_t b;
    if (!mcl_my_row<NT>(rowptr, row0, M, long_rows, long_min, r, b, n)) return;
    uint32_t c = 0;
    for (uint64_t i = threadIdx.x; i < n; i += NT) c += val[b + i] >= thr ? 1u : 0u;
    c = wave_incl_scan(c);
    if (lane_id() == kWave - 1) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += part[w];
        uint32_t kept = s;
        if (n && s == 0) {
            kept = 1;
            atomicAdd(&counters[MCL_RESCUED], 1ull);
        } else if (cap && s > cap) {
            kept = cap;
            atomicAdd(&counters[MCL_CAPPED], 1ull);
        }
        nsurv[r] = s;
        cnt[r] = kept;
    }
}

// ---- the row's sums, division and chaos: ONE wave, whatever the row's class ---------------------------------------------
// vals[0, m) holds the kept entries' inflated values in column order; on return it holds them divided by their sum.
// Returns max(out) - sum(out * out), formed in T (the same value in every lane).
template <class T>
__device__ __forceinline__ T mcl_finish_row(T *__restrict__ vals, uint64_t m) {
#pragma clang fp contract(off)
    const unsigned lane = lane_id();
    const T s = __shfl(wave_ordered_reduce<RED_PLUS>(vals, m), 0, kWave);   // (the order osp_csr_reduce shares)
    T q = T(0), mx = T(0);
    for (uint64_t i = lane; i < m; i += kWave) {
        const T o = vals[i] / s;
        vals[i] = o;
        const T sq = o * o;
        q = q + sq;
        mx = o > mx ? o : mx;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        q = q + __shfl_down(q, d, kWave);
        const T o = __shfl_down(mx, d, kWave);
        mx = o > mx ? o : mx;   // (a maximum does not depend on the order)
    }
    const T c = mx - q;
    return __shfl(c, 0, kWave);
}

// ---- pass 2: select, compact, inflate, normalise ------------------------------------------------------------------------
template <class T, int NT>
__global__ __launch_bounds__(NT) void mcl_write_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                       const T *__restrict__ val, uint64_t row0, uint64_t M,
                                                       const uint32_t *__restrict__ long_rows, uint32_t long_min, T thr, int mode, T power,
                                                       const uint32_t *__restrict__ nsurv, const int64_t *__restrict__ out_ptr,
                                                       uint32_t *__restrict__ out_col, T *__restrict__ out_val,
                                                       unsigned long long *__restrict__ counters) {
    typedef typename MclKey<T>::type K;
    constexpr int NW = NT / kWave;
    constexpr int KBITS = (int)sizeof(K) * 8;
    __shared__ uint32_t hist[NW][kRadix];
    __shared__ uint32_t sel[2][3];        // per pass parity, the chosen bucket: digit, entries above it, entries in it
    __shared__ uint32_t run[2][NW][2];    // per chunk parity and wave: unconditional keeps, entries equal to the k-th value
    uint64_t r, n;
    int64_t b;
    if (!mcl_my_row<NT>(rowptr, row0, M, long_rows, long_min, r, b, n)) return;
    if (n == 0) return;
    const uint64_t ob = (uint64_t)out_ptr[r], m = (uint64_t)out_ptr[r + 1] - ob;
    const unsigned tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t ns = nsurv[r];
    const bool rescue = ns == 0;                 // nothing reaches the threshold: every entry is a candidate, one is kept
    const uint64_t ncand = rescue ? n : ns;
    val += b;
    col += b;

    // keep: candidate && (key >= ge || (key == eq && it is among the first need_eq such entries of the row))
    K ge = 0, eq = 0;
    uint32_t need_eq = 0;
    if (m < ncand) {
        K prefix = 0;
        uint32_t need = (uint32_t)m;
        for (int shift = KBITS - 8, pp = 0;; shift -= 8, pp ^= 1) {
            for (int d = lane; d < kRadix; d += kWave) hist[w][d] = 0;
            if (tid == 0) { sel[pp][0] = 0; sel[pp][1] = 0; sel[pp][2] = 0; }   // (the previous pass's words may still be being read)
            __syncthreads();
            for (uint64_t i = tid; i < n; i += NT) {
                const T v = val[i];
                const K key = mcl_key(v);
                const bool in = (rescue || v >= thr) && (shift == KBITS - 8 || (key >> (shift + 8)) == prefix);
                if (in) atomicAdd(&hist[w][(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < kWave) {   // lane l owns the digits 255 - 4l .. 252 - 4l: descending, so a prefix sum counts what lies above
                uint32_t c[4], tot = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int d = 255 - 4 * (int)lane - j;
                    c[j] = 0;
#pragma unroll
                    for (int ww = 0; ww < NW; ww++) c[j] += hist[ww][d];
                    tot += c[j];
                }
                uint32_t above = wave_incl_scan(tot) - tot;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (above < need && need <= above + c[j]) {
                        sel[pp][0] = 255u - 4u * lane - (uint32_t)j;
                        sel[pp][1] = above;
                        sel[pp][2] = c[j];
                    }
                    above += c[j];
                }
            }
            __syncthreads();
            const uint32_t digit = sel[pp][0], above = sel[pp][1], inside = sel[pp][2];
            need -= above;
            prefix = (K)(prefix << 8) | (K)digit;
            if (need == inside) {   // the bucket is taken whole: no further split
                ge = (K)(prefix << shift);
                need_eq = 0;
                break;
            }
            if (shift == 0) {       // the k-th value itself: everything above it, and the first `need` entries equal to it
                eq = prefix;
                ge = prefix + 1;
                need_eq = need;
                break;
            }
        }
    }

    // one stream over the row: position = (unconditional keeps before me) + min(equal entries before me, need_eq)
    const uint64_t oe = ob + m;
    uint64_t run_gt = 0, run_eq = 0;
    int parity = 0;
    for (uint64_t base = 0; base < n; base += NT, parity ^= 1) {
        const uint64_t i = base + tid;
        T v = T(0);
        uint32_t c = 0;
        bool gt = false, iseq = false;
        if (i < n) {
            v = val[i];
            c = col[i];
            const K key = mcl_key(v);
            const bool cand = rescue || v >= thr;
            gt = cand && key >= ge;
            iseq = cand && !gt && need_eq && key == eq;
        }
        const uint64_t mg = __ballot(gt), me = __ballot(iseq);
        uint64_t gt_before = run_gt + (uint64_t)__popcll(mg & lanemask_lt()), eq_before = run_eq + (uint64_t)__popcll(me & lanemask_lt());
        if constexpr (NW > 1) {
            if (lane == 0) { run[parity][w][0] = (uint32_t)__popcll(mg); run[parity][w][1] = (uint32_t)__popcll(me); }
            __syncthreads();   // (the other parity's words are rewritten only after the next barrier)
#pragma unroll
            for (int ww = 0; ww < NW; ww++) {
                const uint32_t g = run[parity][ww][0], q = run[parity][ww][1];
                if (ww < (int)w) { gt_before += g; eq_before += q; }
                run_gt += g;
                run_eq += q;
            }
        } else {
            run_gt += (uint64_t)__popcll(mg);
            run_eq += (uint64_t)__popcll(me);
        }
        if (gt || (iseq && eq_before < need_eq)) {
            const uint64_t o = ob + gt_before + (eq_before < need_eq ? eq_before : (uint64_t)need_eq);
            if (o < oe) {   // (always, for valid input: unspecified values must still stay inside the row's output)
                out_col[o] = c;
                out_val[o] = mcl_inflate(v, mode, power);
            }
        }
    }
    __syncthreads();
    if (tid < kWave) {
        const T chaos = mcl_finish_row(out_val + ob, m);
        if (lane == 0 && chaos > T(0)) {   // non-negative values: an unsigned maximum of the bit patterns is exact
            if constexpr (sizeof(K) == 8) {
                unsigned long long bits;
                __builtin_memcpy(&bits, &chaos, 8);
                if (bits > __atomic_load_n(&counters[MCL_CHAOS], __ATOMIC_RELAXED)) atomicMax(&counters[MCL_CHAOS], bits);
            } else {
                uint32_t bits;
                __builtin_memcpy(&bits, &chaos, 4);
                if ((unsigned long long)bits > __atomic_load_n(&counters[MCL_CHAOS], __ATOMIC_RELAXED)) atomicMax(&counters[MCL_CHAOS], (unsigned long long)bits);
            }
        }
    }
}

}  // namespace osp
