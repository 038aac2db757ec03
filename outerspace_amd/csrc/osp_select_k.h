// osp_select_k.h -- the row-wise k-select of a CSR result (osp_csr_select_k, include/outerspace_spgemm_select_k.h), written
// for gfx950 (wave64).  DESIGN.md section 31.
//
// Keep, of every row, the k entries that come first under an order.  Every entry gets an unsigned KEY whose ascending order
// is the wanted one (ties: the lower column first):
//   LARGEST / SMALLEST: the value's bits made to order like the value (sign flip), complemented for LARGEST; -0.0 gets the
//                       key of +0.0, every NaN the all-ones key, which no number's key equals.  32 bits for f32, 64 for f64.
//   RANDOM:             mix(s ^ (row << 32 | col)), 64 bits: a bijection of (row, col), so no two entries share a key.
// A row's outcome is a PAIR (t, c): an entry is kept when key < t, or key == t and col <= c.  Rows of at most k entries get
// the pair "everything passes" (all-ones, 2^32 - 1).  Four steps:
//   1. classify: a lane per row writes the pass-all pair and lists the rows longer than k in two classes: up to
//      kSelectKLongMin entries (one wave per row) and beyond (one workgroup of 256 per row).  The lists' order comes from
//      integer atomics and never reaches the result: every row is handled on its own.
//   2. select, listed rows only: a radix select of the k-th key, 8 bits a pass from the top, per-wave histograms in LDS.  It
//      stops as soon as the bucket that holds the k-th key is taken whole (t = the bucket's largest key, c = 2^32 - 1).  When
//      it runs to the last byte, t is the k-th key itself and c the column of the need-th entry with key == t in column
//      order (need = k - the count of smaller keys): one more pass with a prefix count, no sort.  A row is read at most
//      (bytes of the key) + 1 times.
//      The histogram: all-equal rows (and every later pass of a row with many ties) send 64 lanes to ONE counter, which an
//      LDS atomic serialises.  When every lane of a wave that counts at all counts the same digit, one lane adds the
//      population instead (a ballot and a broadcast); mixed digits take the atomic per lane.
//   3. flag: osp_compact.h's flag pass, cut by entries: an entry's row from chunk_entries_and_rows, its key, its row's
//      pair, one verdict bit.  A value order reads each value once here, RANDOM reads none.
//   4. the scan, compact_write_kernel and compact_rowptr_kernel of osp_compact.h, unchanged.
// Every output position is a function of the bit array, and the bit array of the keys alone: no floating-point atomics, no
// wait between workgroups, and nothing depends on the order of processing or on the class boundary.
#pragma once
#include "osp_compact.h"
#include "osp_ewise.h"

namespace osp {

// rows with more entries than this are selected by one workgroup of kSelectKLongThreads, shorter ones by one wave
constexpr uint32_t kSelectKLongMin = 2048;
constexpr int kSelectKLongThreads = 256;
// loads a lane has in flight in a pass over its row.  A wave's row is at most kSelectKLongMin entries: four loads a lane cover
// an eighth of it.  A workgroup's row is streamed by ONE compute unit, whose four waves have nothing else to hide the memory's
// latency behind: sixteen a lane in a histogram pass, eight in the tie pass
constexpr int kSelectKUnroll = 4;
constexpr int kSelectKLongUnroll = 16;
constexpr int kSelectKLongTieUnroll = 8;
// (the values of osp_select_k_order_t)
enum { SELK_LARGEST = 0, SELK_SMALLEST = 1, SELK_RANDOM = 2, SELK_ORDERS = 3 };
// device counters of one call
enum { SELK_NWAVE = 0, SELK_NLONG = 1, SELK_COUNTERS = 2 };

__host__ __device__ __forceinline__ uint64_t select_k_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class T, int ORDER> struct SelectKKey { typedef ValueBits<T> type; };
template <class T> struct SelectKKey<T, SELK_RANDOM> { typedef uint64_t type; };

// the key of a value under LARGEST or SMALLEST
template <class T, int ORDER>
__device__ __forceinline__ ValueBits<T> select_k_value_key(T v) {
    typedef ValueBits<T> K;
    constexpr K ones = ~(K)0, top = (K)1 << (sizeof(K) * 8 - 1);
    if (v != v) return ones;       // every NaN: after every number, equal to one another
    if (v == T(0)) v = T(0);       // (-0.0 orders as +0.0)
    K b;
    __builtin_memcpy(&b, &v, sizeof(K));
    const K asc = (b & top) ? (K)~b : (K)(b | top);   // orders like the value
    return ORDER == SELK_LARGEST ? (K)~asc : asc;
}
// What an entry's key is made from: its value under a value order, its column under RANDOM.  The load and the key are two
// steps so that a lane can issue all the loads of a trip before it uses the first (a key formed inside the bounds check
// made every load wait for the one before: 9 ms a pass over 9 * 10^6 entries).
template <class T, int ORDER> struct SelectKRaw { typedef T type; };
template <class T> struct SelectKRaw<T, SELK_RANDOM> { typedef uint32_t type; };
template <class T, int ORDER>
__device__ __forceinline__ typename SelectKRaw<T, ORDER>::type select_k_load(const uint32_t *__restrict__ col, const T *__restrict__ val, uint64_t p) {
    if constexpr (ORDER == SELK_RANDOM) return col[p];
    else return val[p];
}
// the key of an entry of the row whose hashed number is row_salt = s ^ (row << 32)
template <class T, int ORDER>
__device__ __forceinline__ typename SelectKKey<T, ORDER>::type select_k_key(typename SelectKRaw<T, ORDER>::type raw, uint64_t row_salt) {
    if constexpr (ORDER == SELK_RANDOM) return select_k_mix(row_salt ^ (uint64_t)raw);
    else return select_k_value_key<T, ORDER>(raw);
}

// ---- step 1: the pass-all pair for every row, the rows longer than k in two lists ----------------------------------------------
template <class K>
__global__ __launch_bounds__(256) void select_k_classify_kernel(const int64_t *__restrict__ rowptr, uint64_t M, uint32_t k, uint32_t long_min,
                                                                uint32_t *__restrict__ wave_rows, uint32_t *__restrict__ long_rows,
                                                                unsigned long long *__restrict__ counters, K *__restrict__ thr,
                                                                uint32_t *__restrict__ tie) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t m = 0;
    if (r < M) {
        m = (uint64_t)(rowptr[r + 1] - rowptr[r]);
        thr[r] = ~(K)0;
        tie[r] = 0xffffffffu;
    }
    // one atomic per wave and class: the lanes of a class take consecutive slots behind the leader's
#pragma unroll
    for (int cls = 0; cls < 2; cls++) {
        const bool mine = m > k && (cls == 0 ? m <= long_min : m > long_min);
        const uint64_t mask = __ballot(mine);
        if (mask == 0) continue;
        const int lead = __ffsll((unsigned long long)mask) - 1;
        unsigned long long slot = 0;
        if ((int)lane_id() == lead) slot = atomicAdd(&counters[cls == 0 ? SELK_NWAVE : SELK_NLONG], (unsigned long long)__popcll(mask));
        slot = __shfl(slot, lead, kWave);
        if (mine) (cls == 0 ? wave_rows : long_rows)[slot + (uint64_t)__popcll(mask & lanemask_lt())] = (uint32_t)r;
    }
}

// ---- step 2: the pair of one listed row (more than k entries), by NT threads -----------------------------------------------
template <class T, int ORDER, int NT>
__global__ __launch_bounds__(NT) void select_k_threshold_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                const T *__restrict__ val, const uint32_t *__restrict__ rows, uint32_t k,
                                                                uint64_t s, typename SelectKKey<T, ORDER>::type *__restrict__ thr,
                                                                uint32_t *__restrict__ tie) {
    typedef typename SelectKKey<T, ORDER>::type K;
    typedef typename SelectKRaw<T, ORDER>::type Raw;
    constexpr int NW = NT / kWave;
    constexpr int KBITS = (int)sizeof(K) * 8;
    constexpr int UH = NW == 1 ? kSelectKUnroll : kSelectKLongUnroll, UT = NW == 1 ? 1 : kSelectKLongTieUnroll;
    __shared__ uint32_t hist[NW][kRadix];
    __shared__ uint32_t sel[2][3];         // per pass parity, the chosen bucket: digit, entries below it, entries in it
    __shared__ uint32_t run[2][UT][NW];    // per chunk parity, round and wave: entries equal to the k-th key
    const uint32_t r = rows[blockIdx.x];
    const uint64_t b = (uint64_t)rowptr[r], n = (uint64_t)rowptr[r + 1] - b;   // (n > k >= 1)
    const uint64_t salt = s ^ ((uint64_t)r << 32);
    const unsigned tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    col += b;
    val += b;

    K prefix = 0, t = 0;
    uint32_t need = k;      // of the entries whose key begins with `prefix`, this many smallest are still to be taken
    bool whole = false;
    for (int shift = KBITS - 8, pp = 0;; shift -= 8, pp ^= 1) {
        for (int d = lane; d < kRadix; d += kWave) hist[w][d] = 0;
        if (tid == 0) { sel[pp][0] = 0; sel[pp][1] = 0; sel[pp][2] = 0; }   // (the previous pass's words may still be being read)
        __syncthreads();
        for (uint64_t base = 0; base < n; base += (uint64_t)UH * NT) {   // (the same trips in every lane)
            Raw raw[UH];
#pragma unroll
            for (int u = 0; u < UH; u++) {   // (past the end: the row's last entry again, not counted)
                const uint64_t i = base + (uint64_t)u * NT + tid;
                raw[u] = select_k_load<T, ORDER>(col, val, i < n ? i : n - 1);
            }
#pragma unroll
            for (int u = 0; u < UH; u++) {
                const K key = select_k_key<T, ORDER>(raw[u], salt);
                const bool cnt = base + (uint64_t)u * NT + tid < n && (shift == KBITS - 8 || (key >> (shift + 8)) == prefix);
                const unsigned digit = (unsigned)(key >> shift) & 255u;
                const uint64_t mask = __ballot(cnt);
                if (mask == 0) continue;
                const int lead = __ffsll((unsigned long long)mask) - 1;
                const unsigned d0 = (unsigned)__shfl((int)digit, lead, kWave);
                if (__ballot(cnt && digit == d0) == mask) {   // one digit in the whole wave: one lane adds the population
                    if ((int)lane == lead) atomicAdd(&hist[w][d0], (uint32_t)__popcll(mask));
                } else if (cnt) {
                    atomicAdd(&hist[w][digit], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < kWave) {   // lane l owns the digits 4l .. 4l + 3: ascending, so a prefix sum counts what lies below
            uint32_t c[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c[j] = 0;
#pragma unroll
                for (int ww = 0; ww < NW; ww++) c[j] += hist[ww][4 * lane + j];
                tot += c[j];
            }
            uint32_t below = wave_incl_scan(tot) - tot;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (below < need && need <= below + c[j]) {
                    sel[pp][0] = 4u * lane + (uint32_t)j;
                    sel[pp][1] = below;
                    sel[pp][2] = c[j];
                }
                below += c[j];
            }
        }
        __syncthreads();
        const uint32_t digit = sel[pp][0], below = sel[pp][1], inside = sel[pp][2];
        need -= below;
        prefix = (K)(prefix << 8) | (K)digit;
        if (need == inside) {   // the bucket is taken whole: every key up to its largest passes
            t = (K)(prefix << shift) | (K)(((K)1 << shift) - 1);
            whole = true;
            break;
        }
        if (shift == 0) {       // the k-th key itself: everything below it, and the first `need` entries equal to it
            t = prefix;
            break;
        }
    }
    if (tid == 0) {
        thr[r] = t;
        if (whole) tie[r] = 0xffffffffu;
    }
    if (whole) return;

    // the column of the need-th entry with key == t, in column order: a prefix count over the row
    uint32_t seen = 0;   // (the same in every thread)
    int parity = 0;
    for (uint64_t base = 0; base < n; base += (uint64_t)UT * NT, parity ^= 1) {   // round u holds the entries base + u NT + tid
        Raw raw[UT];
        bool eq[UT];
        uint32_t before[UT];   // equal entries before mine in my wave's part of my round
#pragma unroll
        for (int u = 0; u < UT; u++) {
            const uint64_t i = base + (uint64_t)u * NT + tid;
            raw[u] = select_k_load<T, ORDER>(col, val, i < n ? i : n - 1);
        }
#pragma unroll
        for (int u = 0; u < UT; u++) eq[u] = base + (uint64_t)u * NT + tid < n && select_k_key<T, ORDER>(raw[u], salt) == t;
#pragma unroll
        for (int u = 0; u < UT; u++) {
            const uint64_t m = __ballot(eq[u]);
            before[u] = (uint32_t)__popcll(m & lanemask_lt());
            if constexpr (NW > 1) {
                if (lane == 0) run[parity][u][w] = (uint32_t)__popcll(m);
            } else {
                if (eq[u] && seen + before[u] == need - 1) tie[r] = col[base + tid];
                seen += (uint32_t)__popcll(m);
            }
        }
        if constexpr (NW > 1) {
            __syncthreads();   // (the other parity's words are rewritten only after the next barrier)
#pragma unroll
            for (int u = 0; u < UT; u++) {
                uint32_t mine = seen + before[u];
#pragma unroll
                for (int ww = 0; ww < NW; ww++) {
                    const uint32_t q = run[parity][u][ww];
                    if (ww < (int)w) mine += q;
                    seen += q;
                }
                if (eq[u] && mine == need - 1) tie[r] = col[base + (uint64_t)u * NT + tid];
            }
        }
        if (seen >= need) break;
    }
}

// ---- step 3: one verdict bit per entry ------------------------------------------------------------------------------------------
template <class T, int ORDER>
__global__ __launch_bounds__(kCompactThreads) void select_k_flag_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                        const T *__restrict__ val, uint64_t M, uint64_t nnz, uint64_t s,
                                                                        const typename SelectKKey<T, ORDER>::type *__restrict__ thr,
                                                                        const uint32_t *__restrict__ tie, uint64_t *__restrict__ bits) {
    typedef typename SelectKKey<T, ORDER>::type K;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    T v[kCompactRounds];
    if constexpr (ORDER != SELK_RANDOM) {   // (issued before the row searches)
#pragma unroll
        for (int q = 0; q < kCompactRounds; q++) {
            const uint64_t e = base + (uint64_t)q * kCompactThreads + threadIdx.x;
            v[q] = e < nnz ? val[e] : T(0);
        }
    }
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int q = 0; q < kCompactRounds; q++) {
        const bool valid = (uint64_t)p[q] < nnz;
        const uint32_t row = lo[q] - 1;   // (past the end: the chunk's first row, whose pair exists)
        K key;
        if constexpr (ORDER == SELK_RANDOM) key = select_k_mix(s ^ ((uint64_t)row << 32) ^ (uint64_t)j[q]);
        else key = select_k_value_key<T, ORDER>(v[q]);
        const K t = thr[row];
        const uint32_t c = tie[row];
        store_verdicts(valid && (key < t || (key == t && j[q] <= c)), (uint64_t)p[q], nnz, bits);
    }
}

}  // namespace osp
