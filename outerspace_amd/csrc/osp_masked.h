// osp_masked.h -- the masked product C<M> = A*B (osp_spgemm_masked, include/outerspace_spgemm_masked.h), written for gfx950
// (wave64).  DESIGN.md section 9.
//
// Dot-product formulation: C[i,j], for (i, j) in the mask, is the intersection of row i of A with column j of B, both
// ascending in k, summed in ascending k.  The outer-product pipeline (staging, sort, merge tiles) is not involved:
//   1. views: A in (row, k) order and B in (col, k) order, one stable radix sort each (osp_sort.h) -- the input is already
//      ascending in k inside every segment, so sorting by the new major index alone keeps k ascending;
//   2. every mask entry ("slot") is classified by its list lengths la = |A row i|, lb = |B col j|: no work (either is 0),
//      light, or heavy (min(la, lb) > kMaskedHeavyMin); light slots are ordered by a log2 cost bucket (one 5-bit pass of
//      the same radix sort) so that the lanes of a wave carry similar walks;
//   3. light slots: one lane per slot walks the shorter list and gallops in the longer one;
//      heavy slots: one wave per slot, the shorter list cut into rounds of 64 contiguous pieces;
//   4. a hit flag and a value per slot, an exclusive scan over the flags, and C at its exact size.
//
// Bit-exactness against the reference's deduplicateCOO (SimSpGEMM.cpp:519-535), which sums every (i, j) left to right in
// ascending k starting from the first product: every slot's sum starts at -0.0 (-0.0 + x == x for every x, where +0.0
// would turn a lone -0.0 product into +0.0), adds its products one at a time in ascending k, and is never contracted
// (an FMA rounds once where the reference rounds twice): `#pragma clang fp contract(off)` in every accumulating function.
// Per-lane partial sums of a heavy slot are never combined: one lane adds the whole k-ordered sequence.
#pragma once
#include "osp_sort.h"
#include "osp_epilogue.h"

namespace osp {

// A slot is heavy when min(la, lb) exceeds this (OSP_MASKED_HEAVY_MIN overrides it for measurement; MEASUREMENTS.md
// section 0b records the choice).
constexpr uint32_t kMaskedHeavyMin = 2048;
// entries of the shorter list one lane of a heavy slot's wave takes per round: a round covers 64 * kMaskedHeavyChunk
constexpr int kMaskedHeavyChunk = 32;
// slot classes as sort keys: 0 = no work, 1..30 = light (cost bucket), 31 = heavy
constexpr uint32_t kMaskedEmpty = 0, kMaskedHeavy = 31, kMaskedBuckets = 32;

// ---- views: the last pass of device_sort_rows writes (major, minor, value) in (major, k) order --------------------------
template <class T>
struct MaskedViewEpilogue {
    const uint32_t *minor;   // k of the input entry e (A: its CSC column, B: its CSR row)
    const T *vals;
    uint32_t *major_out, *minor_out;
    T *vals_out;
    __device__ void operator()(uint64_t t, uint32_t major, uint32_t e) const {
        major_out[t] = major;
        minor_out[t] = minor[e];
        vals_out[t] = vals[e];
    }
};

// the payload alone: order[t] = the slot at sorted position t
struct MaskedOrderEpilogue {
    uint32_t *order;
    __device__ void operator()(uint64_t t, uint32_t, uint32_t slot) const { order[t] = slot; }
};

// ---- classification ---------------------------------------------------------------------------------------------------
// key[s] = the slot's class (above), hit[s] = 0; count[class] += 1 (per-workgroup histogram, then 32 atomics)
__global__ __launch_bounds__(256) void masked_classify_kernel(const uint32_t *__restrict__ m_row, const uint32_t *__restrict__ m_colidx,
                                                              const int64_t *__restrict__ arow_ptr, const int64_t *__restrict__ bcol_ptr,
                                                              uint64_t nnz_m, uint32_t heavy_min, int bucketed, uint32_t *__restrict__ key,
                                                              uint32_t *__restrict__ hit, uint32_t *__restrict__ count) {
    __shared__ uint32_t h[kMaskedBuckets];
    if (threadIdx.x < kMaskedBuckets) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nnz_m) {
        const uint32_t i = m_row[s], j = m_colidx[s];
        const uint64_t la = (uint64_t)(arow_ptr[i + 1] - arow_ptr[i]), lb = (uint64_t)(bcol_ptr[j + 1] - bcol_ptr[j]);
        const uint64_t lo = min(la, lb), hi = max(la, lb);
        uint32_t c;
        if (lo == 0) c = kMaskedEmpty;
        else if (lo > heavy_min) c = kMaskedHeavy;
        else if (!bucketed) c = 1;
        else {
            // cost ~ lo * log2(hi / lo + 1): a gallop per entry of the shorter list
            const uint64_t cost = lo * (uint64_t)(64 - __clzll(hi / lo));
            c = 1u + min(29u, (uint32_t)(63 - __clzll(cost)));
        }
        key[s] = c;
        hit[s] = 0;
        atomicAdd(&h[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kMaskedBuckets && h[threadIdx.x]) atomicAdd(&count[threadIdx.x], h[threadIdx.x]);
}

// ---- intersection walks -----------------------------------------------------------------------------------------------
// First index in [lo, n) with a[idx] >= x, or n: an exponential step from the cursor, then bisection.
__device__ __forceinline__ uint64_t gallop_lower_bound(const uint32_t *a, uint64_t lo, uint64_t n, uint32_t x) {
    if (lo >= n || a[lo] >= x) return lo;
    uint64_t step = 1;   // invariant: a[lo] < x
    while (lo + step < n && a[lo + step] < x) {
        lo += step;
        step <<= 1;
    }
    uint64_t hi = min(lo + step, n);   // a[hi] >= x, or hi == n
    lo++;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One lane: the shorter list (sk, sv) against the longer (lk, lv); acc += a * b for every common k, in ascending k.  SWAP:
// the shorter list is B's column (the product stays A's value times B's).  Returns the number of products.
template <class T, bool SWAP>
__device__ __forceinline__ uint32_t masked_walk(const uint32_t *sk, const T *sv, uint64_t ls, const uint32_t *lk, const T *lv, uint64_t ll,
                                                T &acc) {
#pragma clang fp contract(off)
    uint32_t hits = 0;
    uint64_t c = 0;
    for (uint64_t p = 0; p < ls; p++) {
        const uint32_t x = sk[p];
        c = gallop_lower_bound(lk, c, ll, x);
        if (c == ll) break;
        if (lk[c] == x) {
            const T a = SWAP ? lv[c] : sv[p], b = SWAP ? sv[p] : lv[c];
            const T prod = a * b;
            acc = acc + prod;
            hits++;
            c++;
        }
    }
    return hits;
}

struct MaskedOperands {
    const uint32_t *m_row, *m_colidx;   // slot s = (m_row[s], m_colidx[s])
    const int64_t *arow_ptr;            // A's row view: M + 1 offsets, k, values
    const uint32_t *arow_k;
    const int64_t *bcol_ptr;            // B's column view: N + 1 offsets, k, values
    const uint32_t *bcol_k;
};

// Light slots order[0, n): one lane per slot.  hit[s] = 1 when the slot has a product, val[s] = its sum; *products += the
// products formed.
template <class T>
__global__ __launch_bounds__(256) void masked_light_kernel(const MaskedOperands op, const T *__restrict__ arow_v, const T *__restrict__ bcol_v,
                                                           const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ hit,
                                                           T *__restrict__ val, unsigned long long *products) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t hits = 0;
    if (t < n) {
        const uint32_t s = order[t];
        const uint32_t i = op.m_row[s], j = op.m_colidx[s];
        const int64_t a0 = op.arow_ptr[i], b0 = op.bcol_ptr[j];
        const uint64_t la = (uint64_t)(op.arow_ptr[i + 1] - a0), lb = (uint64_t)(op.bcol_ptr[j + 1] - b0);
        T acc = (T)-0.0;
        if (la <= lb) hits = masked_walk<T, false>(op.arow_k + a0, arow_v + a0, la, op.bcol_k + b0, bcol_v + b0, lb, acc);
        else hits = masked_walk<T, true>(op.bcol_k + b0, bcol_v + b0, lb, op.arow_k + a0, arow_v + a0, la, acc);
        hit[s] = hits ? 1u : 0u;
        val[s] = acc;
    }
    const uint32_t w = wave_incl_scan(hits);
    if (lane_id() == kWave - 1 && w) atomicAdd(products, (unsigned long long)w);
}

// Heavy slots order[0, n): one wave (one 64-thread workgroup) per slot.  Round by round, the next 64 * kMaskedHeavyChunk
// entries of the shorter list are cut into 64 contiguous pieces, one per lane; every lane bisects to its piece's start in
// the longer list (from where the previous round ended), gallops through its piece and writes its products, in k order,
// to its own stripe of an LDS buffer.  The stripes in lane order are the round's products in ascending k; lane 0 adds
// them one by one to the carried sum.
template <class T>
__global__ __launch_bounds__(kWave) void masked_heavy_kernel(const MaskedOperands op, const T *__restrict__ arow_v, const T *__restrict__ bcol_v,
                                                             const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ hit,
                                                             T *__restrict__ val, unsigned long long *products) {
#pragma clang fp contract(off)
    __shared__ T buf[kWave * kMaskedHeavyChunk];
    __shared__ uint32_t cnt[kWave];
    const uint64_t t = blockIdx.x;
    if (t >= n) return;
    const unsigned lane = lane_id();
    const uint32_t s = order[t];
    const uint32_t i = op.m_row[s], j = op.m_colidx[s];
    const int64_t a0 = op.arow_ptr[i], b0 = op.bcol_ptr[j];
    const uint64_t la = (uint64_t)(op.arow_ptr[i + 1] - a0), lb = (uint64_t)(op.bcol_ptr[j + 1] - b0);
    const bool swap = lb < la;   // (wave-uniform)
    const uint32_t *sk = swap ? op.bcol_k + b0 : op.arow_k + a0, *lk = swap ? op.arow_k + a0 : op.bcol_k + b0;
    const T *sv = swap ? bcol_v + b0 : arow_v + a0, *lv = swap ? arow_v + a0 : bcol_v + b0;
    const uint64_t ls = swap ? lb : la, ll = swap ? la : lb;
    T acc = (T)-0.0;
    uint64_t total = 0, from = 0;   // `from`: where the previous round ended in the longer list
    for (uint64_t base = 0; base < ls && from < ll; base += (uint64_t)kWave * kMaskedHeavyChunk) {
        const uint64_t p0 = base + (uint64_t)lane * kMaskedHeavyChunk, p1 = min(p0 + kMaskedHeavyChunk, ls);
        uint64_t c = ll;
        uint32_t h = 0;
        if (p0 < ls) {
            c = lower_bound_dev(lk, from, ll, sk[p0]);
            for (uint64_t p = p0; p < p1 && c < ll; p++) {
                const uint32_t x = sk[p];
                c = gallop_lower_bound(lk, c, ll, x);
                if (c == ll) break;
                if (lk[c] == x) {
                    const T a = swap ? lv[c] : sv[p], b = swap ? sv[p] : lv[c];
                    buf[lane * kMaskedHeavyChunk + h] = a * b;
                    h++;
                    c++;
                }
            }
        }
        cnt[lane] = h;
        total += wave_reduce_sum_u62((uint64_t)h);
        from = (uint64_t)__shfl(c, kWave - 1, kWave);   // the last lane's cursor: every later piece starts at or beyond it
        __syncthreads();
        if (lane == 0) {
            for (int l = 0; l < kWave; l++) {
                const uint32_t nl = cnt[l];
                for (uint32_t q = 0; q < nl; q++) acc = acc + buf[l * kMaskedHeavyChunk + q];
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        hit[s] = total ? 1u : 0u;
        val[s] = acc;
        if (total) atomicAdd(products, (unsigned long long)total);
    }
}

// ---- compaction -------------------------------------------------------------------------------------------------------
// rowptr[i] = pos[m_rowptr[i]] for i in [0, M]
__global__ void masked_rowptr_kernel(const int64_t *__restrict__ m_rowptr, const uint64_t *__restrict__ pos, uint64_t M, int64_t *__restrict__ rowptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= M) rowptr[i] = (int64_t)pos[m_rowptr[i]];
}
template <class T>
__global__ void masked_scatter_kernel(const uint32_t *__restrict__ hit, const T *__restrict__ val, const uint32_t *__restrict__ m_colidx,
                                      const uint64_t *__restrict__ pos, uint64_t nnz_m, uint32_t *__restrict__ colidx, T *__restrict__ vals) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nnz_m && hit[s]) {
        const uint64_t q = pos[s];
        colidx[q] = m_colidx[s];
        vals[q] = val[s];
    }
}

}  // namespace osp
