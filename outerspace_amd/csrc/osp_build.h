// osp_build.h -- a CSR result from a COO list whose repeated coordinates are combined by an operator in LIST order, written
// for gfx950 (wave64): the kernels of osp_csr_build (include/outerspace_spgemm_build.h).  DESIGN.md section 19.
//
// The list is ordered by the two stable sorts of osp_spgemm_coo's ingest (osp_sort.h: by column, then by row), which leave
// the sorted rows, and the permutation perm[t] = the list position of sorted entry t.  Stable means that a RUN -- the entries
// of one coordinate -- lies contiguous and in list order.  After the sorts:
//   1. heads:  one verdict bit per sorted entry (osp_compact.h's bit array): entry t begins a run when t == 0 or its
//              (row, column) differs from entry t - 1's.  An index beyond its dimension raises the error word here; it has
//              only ever been a sort key.
//   2. scan, row pointer: osp_compact.h's, over the sorted list's row pointer
//   3. write:  only a head works.  Its place is the compaction's, its run's length the distance to the next set bit -- the
//              rest of its own word, the next word, and beyond that a bisection of the scan for the word that holds head
//              number o + 1: keys are not compared again.  Values come from the caller's array through perm, and only
//              those the operator needs.
// Work is cut by sorted ENTRIES, kCompactChunk a workgroup, never by rows or runs.  A run of up to kBuildLongRun entries
// is folded by its head's lane, one after the other; a longer one (under PLUS, MIN, MAX with values) by the head's whole
// wave: 64 values loaded coalesced through perm, then the 64 dependent operations in order, every lane computing the same
// chain from the values the others hold (build_fold_wave).  Both paths apply the same operations in the same order, so where
// a run lies and which path folds it does not show in the result.  A long run belongs to the workgroup of its head, however
// many chunks it crosses.
// No float atomics, no waiting between workgroups; the atomics are the integer OR of the error word and the integer count
// of long runs.  The operator is a template parameter: there is no branch on it in a kernel.
#pragma once
#include "osp_compact.h"
#include "osp_ewise.h"

namespace osp {

// (the values of osp_dup_op_t)
enum { DUP_ERROR = 0, DUP_PLUS, DUP_MIN, DUP_MAX, DUP_FIRST, DUP_LAST, DUP_COUNT, DUP_OPS };

constexpr uint32_t kBuildLongRun = 64;   // a run of more entries than this is folded by a wave
constexpr uint32_t kBuildBadIndex = 1u;  // bit of the error word

// ---- 1: one verdict per sorted entry: does it begin a run ----------------------------------------------------------------------
__global__ __launch_bounds__(kCompactThreads) void build_heads_kernel(const uint32_t *__restrict__ row, const uint32_t *__restrict__ col, uint64_t nnz,
                                                                      uint64_t M, uint64_t N, uint64_t *__restrict__ bits, uint32_t *err) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kCompactThreads + threadIdx.x;
        bool head = false;
        if (p < nnz) {
            const uint32_t r = row[p], c = col[p];
            bad |= r >= M || c >= N;
            head = p == 0 || row[p - 1] != r || col[p - 1] != c;
        }
        store_verdicts(head, p, nnz, bits);
    }
    if (__ballot(bad) && lane_id() == 0) atomicOr(err, kBuildBadIndex);
}

// ---- 3: the runs' columns and folded values at their positions ------------------------------------------------------------------
// The entry after the last of the run whose head is entry t, bit t & 63 of `word`, head number o of nnz_out.
__device__ __forceinline__ uint64_t build_run_end(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos, uint64_t nwords, uint64_t nnz,
                                                  uint64_t nnz_out, uint64_t t, uint64_t word, uint64_t o) {
    const unsigned b = (unsigned)(t & 63);
    const uint64_t above = b == 63 ? 0ull : word >> (b + 1);
    if (above) return t + (uint64_t)__ffsll((unsigned long long)above);
    const uint64_t w = (t >> 6) + 1;
    if (o + 1 == nnz_out) return nnz;   // the last run (w may not exist)
    const uint64_t next = bits[w];
    if (next) return w * 64 + (uint64_t)__ffsll((unsigned long long)next) - 1;
    // the word that holds head o + 1: the first x with pos[x + 1] >= o + 2 (it exists: this is not the last run)
    const uint64_t x = lower_bound_dev(pos + 1, w + 1, nwords, o + 2);
    return x * 64 + (uint64_t)__ffsll((unsigned long long)bits[x]) - 1;
}

// lane i's `v` in every lane, i a constant: a scalar read of the register (v_readlane), where __shfl goes through the LDS
// crossbar -- and the chain below waits for each of its 64 values in turn
template <class V>
__device__ __forceinline__ V build_lane_value(V v, int i) {
    if constexpr (sizeof(V) == 4) {
        return (V)__builtin_amdgcn_readlane((int)v, i);
    } else {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), i);
        return ((V)hi << 32) | lo;
    }
}
// acc (+) the `cnt` values the wave's lanes 0 .. cnt - 1 hold, in lane order; FROM: the first lane taken (1: lane 0's value
// is acc already).  The same chain in every lane.
template <class T, int EW, int FROM, class V>
__device__ __forceinline__ V build_fold_block(V acc, V mine, unsigned cnt) {
    if (cnt == (unsigned)kWave) {
#pragma unroll
        for (int i = FROM; i < kWave; i++) acc = ewise_apply<EW, T, V>(acc, build_lane_value(mine, i));
    } else {
        for (unsigned i = FROM; i < cnt; i++) acc = ewise_apply<EW, T, V>(acc, __shfl(mine, (int)i));
    }
    return acc;
}
// The fold of the run of sorted entries [t0, e), e - t0 > kWave, by a whole wave (t0 and e the same in every lane): 64 values
// at a time, the next 64 on their way while these are combined.  Every lane returns the result.
template <class T, int EW, class V>
__device__ __forceinline__ V build_fold_wave(const uint32_t *__restrict__ perm, const V *__restrict__ vals, uint64_t t0, uint64_t e) {
    const unsigned lane = lane_id();
    V mine = vals[perm[t0 + lane]];   // (the first 64 exist)
    V acc = __shfl(mine, 0);
    bool first = true;
    for (uint64_t t = t0;;) {
        const uint64_t tn = t + kWave;
        V next = 0;
        if (tn + lane < e) next = vals[perm[tn + lane]];
        const unsigned cnt = e - t < (uint64_t)kWave ? (unsigned)(e - t) : (unsigned)kWave;
        acc = first ? build_fold_block<T, EW, 1>(acc, mine, cnt) : build_fold_block<T, EW, 0>(acc, mine, cnt);
        first = false;
        if (tn >= e) break;
        t = tn;
        mine = next;
    }
    return acc;
}

// the value of a run of m entries every one of which is 1 (vals NULL), or their number (COUNT)
template <class T, int OP>
__device__ __forceinline__ ValueBits<T> build_ones(uint64_t m) {
    T v = (T)1;
    if (OP == DUP_COUNT) v = (T)m;
    // the chain 1 + 1 + ...: exact while the sum has a successor, then it stays (f32: at 2^24; f64: beyond any list)
    if (OP == DUP_PLUS) v = sizeof(T) == 4 && m > (1ull << 24) ? (T)(1ull << 24) : (T)m;
    return ewise_as_bits<ValueBits<T>>(v);
}

// OP: DUP_PLUS, DUP_MIN, DUP_MAX, DUP_FIRST (also for DUP_ERROR: every run has one entry then), DUP_LAST, DUP_COUNT.
// VALS: the values are read (never for COUNT); else every value is 1 (OP: DUP_PLUS, DUP_COUNT, or DUP_FIRST for the rest).
template <class T, int OP, bool VALS>
__global__ __launch_bounds__(kCompactThreads) void build_write_kernel(const uint32_t *__restrict__ col, const uint32_t *__restrict__ perm,
                                                                      const ValueBits<T> *__restrict__ vals, uint64_t nnz, uint64_t nnz_out,
                                                                      const uint64_t *__restrict__ bits, const uint64_t *__restrict__ pos,
                                                                      uint32_t *__restrict__ out_col, ValueBits<T> *__restrict__ out_val,
                                                                      unsigned long long *n_long) {
    typedef ValueBits<T> V;
    constexpr bool FOLDS = VALS && (OP == DUP_PLUS || OP == DUP_MIN || OP == DUP_MAX);
    constexpr int EW = OP == DUP_MIN ? EW_MIN : OP == DUP_MAX ? EW_MAX : EW_PLUS;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    const uint64_t nwords = (nnz + 63) / 64;
    uint32_t longs_seen = 0;
    for (int k = 0; k < kCompactRounds; k++) {
        const uint64_t p = base + (uint64_t)k * kCompactThreads + threadIdx.x;
        bool head = false, is_long = false;
        uint64_t o = 0, e = 0;
        if (p < nnz) {
            const uint64_t word = bits[p >> 6];
            head = (word >> (p & 63)) & 1ull;
            if (head) {
                o = pos[p >> 6] + (uint64_t)__popcll(word & ((1ull << (p & 63)) - 1ull));
                e = build_run_end(bits, pos, nwords, nnz, nnz_out, p, word, o);
            }
        }
        if (head) {
            out_col[o] = col[p];
            const uint64_t m = e - p;
            if constexpr (FOLDS) {
                is_long = m > kBuildLongRun;
                if (!is_long) {
                    V acc = vals[perm[p]];
                    for (uint64_t i = 1; i < m; i++) acc = ewise_apply<EW, T, V>(acc, vals[perm[p + i]]);
                    out_val[o] = acc;
                }
            } else if constexpr (VALS) {
                out_val[o] = vals[perm[OP == DUP_LAST ? e - 1 : p]];
            } else {
                out_val[o] = build_ones<T, OP>(m);
            }
        }
        if constexpr (FOLDS) {   // the long runs of this round, one after the other, each by the whole wave
            uint64_t longs = __ballot(is_long);
            longs_seen += (uint32_t)__popcll(longs);
            while (longs) {
                const int l = __ffsll((unsigned long long)longs) - 1;
                longs &= longs - 1;
                const uint64_t t0 = __shfl((unsigned long long)p, l), e0 = __shfl((unsigned long long)e, l);
                const V acc = build_fold_wave<T, EW, V>(perm, vals, t0, e0);
                if (lane_id() == (unsigned)l) out_val[o] = acc;
            }
        }
    }
    if constexpr (FOLDS)
        if (longs_seen && lane_id() == 0) atomicAdd(n_long, (unsigned long long)longs_seen);
}

}  // namespace osp
