// osp_scan.h -- the row-wise inclusive scan of a CSR result and the weighted draws from its rows (osp_csr_scan, osp_csr_draw,
// include/outerspace_spgemm_scan.h), written for gfx950 (wave64).  DESIGN.md section 32.
//
// The scan's order is part of the interface (the header states it in full): a row is cut into blocks of kScanBlock = 32
// entries, L is the sequential scan inside a block, T_b the block's last L, C_b the sequential scan of the T's of the row's
// earlier blocks, S_q = C_b (+) L_q.  Two levels and no more: that order is monotone on non-negative input in floating point,
// which a scan by doubling inside a wave is not, and a draw's bisection of the CDF needs it.  Four steps:
//   1. the block table: the blocks of every row, ceil(m / 32), scanned by the library's exclusive scan into blkptr[0 .. M].
//      The kernels below are launched for the host's bound nnz / 32 + M of the blocks, and lanes beyond blkptr[M] leave:
//      nothing is read back.
//   2. scan_local_kernel: a lane owns one block.  The blocks of a workgroup are consecutive, so their entries are ONE
//      consecutive piece of the arrays (rows without entries own no block): the workgroup loads it with consecutive lanes on
//      consecutive entries into LDS, every lane runs its 32 sequential steps there, and the piece goes out the same way.  Entry x
//      of the piece lies at word x + x / 32: lane t of full blocks then reads word 33 t + q at step q, a different bank in
//      every lane of a half wave, for 4-byte and for 8-byte values.  A lane's row is a bisection of the block table between
//      the rows of its wave's first and last block, which the wave finds once with 64 probes a step (as osp_kron.h does).
//      T_b goes to a temporary.  The entries come from a SOURCE in the sense of osp_vector.h: Values for the scan, Weights
//      (the draw's weight transform) for the CDF.
//   3. scan_chain_kernel: C_b for the rows of more than one block, sequential per row by definition.  A lane per row up to
//      kScanChainLane blocks; longer rows one after another by the whole wave, which loads 64 block totals at once and walks
//      them through lane reads.
//   4. scan_add_kernel: cut by entries (an entry's row from the bisections of osp_compact.h): S_q = C_b (+) L_q in place for
//      the entries of the blocks b >= 1.
// The draw: a lane per (row, draw) hashes (seed, row, draw), multiplies by the row's total and bisects the row's slice of S.
// No floating-point atomics, no wait between workgroups: every output is a function of its row's values alone.
#pragma once
#include "osp_compact.h"
#include "osp_vector.h"
#include "osp_select_k.h"

namespace osp {

constexpr uint32_t kScanBlock = 32;                   // (OSP_SCAN_BLOCK)
constexpr int kScanLocalThreads = 128;                // blocks of one workgroup of the local pass
constexpr uint32_t kScanPitch = kScanBlock + 1;       // words of LDS per 32 entries
constexpr uint64_t kScanChainLane = 16;               // rows of more blocks than this are chained by a whole wave
constexpr unsigned kDrawBlocks = 1u << 20;            // the draw kernel strides over (row, draw) with at most this many blocks

// the blocks of row i
struct LoadRowBlocks {
    const int64_t *rowptr;
    __device__ uint64_t operator()(uint64_t i) const { return ((uint64_t)(rowptr[i + 1] - rowptr[i]) + kScanBlock - 1) / kScanBlock; }
};

// the draw's weight transform as a source: zeros, negatives, NaNs and infinities weigh +0.0
template <class T>
struct Weights {
    const T *vals;
    __device__ __forceinline__ T value(uint64_t i) const {
        const T e = vals[i];
        return e > T(0) && e < (T)__builtin_inf() ? e : T(0);
    }
};

__device__ __forceinline__ uint32_t scan_word(uint32_t x) { return x + x / kScanBlock; }

// lane j's value in every lane (j the same in every lane)
template <class T>
__device__ __forceinline__ T wave_read_lane(T v, int j) {
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); k++) w[k] = __builtin_amdgcn_readlane(w[k], j);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// ---- step 2: L of every entry into out, T of every block into totals ----------------------------------------------------------------
template <class T, int OP, class Src>
__global__ __launch_bounds__(kScanLocalThreads) void scan_local_kernel(const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ blkptr, uint64_t M,
                                                                       Src src, T *__restrict__ out, T *__restrict__ totals) {
    __shared__ T tile[kScanLocalThreads * kScanPitch];
    __shared__ uint64_t span[2];   // the workgroup's entries [span[0], span[1])
    const uint64_t nb = blkptr[M];
    const uint64_t first = (uint64_t)blockIdx.x * kScanLocalThreads;
    if (first >= nb) return;       // (the grid covers the host's upper bound of the blocks)
    const uint64_t end = first + kScanLocalThreads < nb ? first + kScanLocalThreads : nb;
    const uint64_t blk = first + threadIdx.x, wave_first = first + (threadIdx.x & ~63u);
    uint64_t start = 0;
    uint32_t len = 0;
    if (wave_first < end) {        // (the same in every lane of a wave)
        const uint64_t wave_last = (wave_first + kWave < end ? wave_first + kWave : end) - 1;
        // the last row r with blkptr[r] <= block holds the block: among equal pointers, the one with entries
        const uint64_t r_first = wave_upper_bound(blkptr, 0, M + 1, wave_first) - 1;
        const uint64_t r_last = wave_upper_bound(blkptr, r_first + 1, M + 1, wave_last) - 1;
        if (blk < end) {
            const uint64_t r = r_first == r_last ? r_first : upper_bound_dev(blkptr, r_first + 1, r_last + 1, blk) - 1;
            start = (uint64_t)rowptr[r] + (blk - blkptr[r]) * kScanBlock;
            const uint64_t left = (uint64_t)rowptr[r + 1] - start;   // (at least 1: the row owns this block)
            len = left < kScanBlock ? (uint32_t)left : kScanBlock;
            if (blk == first) span[0] = start;
            if (blk == end - 1) span[1] = start + len;
        }
    }
    __syncthreads();
    const uint64_t e0 = span[0];
    const uint32_t n = (uint32_t)(span[1] - e0);   // (at most kScanLocalThreads * kScanBlock)
#pragma unroll 4
    for (uint32_t x = threadIdx.x; x < n; x += kScanLocalThreads) tile[scan_word(x)] = src.value(e0 + x);
    __syncthreads();
    if (len) {
        const uint32_t x0 = (uint32_t)(start - e0);
        T acc = ordered_identity<OP, T>();
        for (uint32_t q = 0; q < len; q++) {
            const uint32_t w = scan_word(x0 + q);
            acc = ordered_combine<OP>(acc, tile[w]);
            tile[w] = acc;
        }
        totals[blk] = acc;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t x = threadIdx.x; x < n; x += kScanLocalThreads) out[e0 + x] = tile[scan_word(x)];
}

// ---- step 3: carry[b] = C of block b, for the blocks b >= 1 of every row ------------------------------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(256) void scan_chain_kernel(const uint64_t *__restrict__ blkptr, uint64_t M, const T *__restrict__ totals,
                                                         T *__restrict__ carry) {
    const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = lane_id();
    uint64_t b0 = 0, nblk = 0;
    if (row < M) {
        b0 = blkptr[row];
        nblk = blkptr[row + 1] - b0;
    }
    if (nblk > 1 && nblk <= kScanChainLane) {
        T c = ordered_identity<OP, T>();
        for (uint64_t b = 1; b < nblk; b++) {
            c = ordered_combine<OP>(c, totals[b0 + b - 1]);
            carry[b0 + b] = c;
        }
    }
    // the longer rows of this wave's 64, one after another by the whole wave
    for (uint64_t longs = __ballot(nblk > kScanChainLane); longs; longs &= longs - 1) {
        const int l = __ffsll((unsigned long long)longs) - 1;
        const uint64_t rb = (uint64_t)__shfl((long long)b0, l, kWave), rn = (uint64_t)__shfl((long long)nblk, l, kWave);
        T c = ordered_identity<OP, T>();   // (the same in every lane)
        for (uint64_t base = 0; base < rn; base += kWave) {
            // (past the row's end: the identity, which changes no carry)
            const T t = base + lane < rn ? totals[rb + base + lane] : ordered_identity<OP, T>();
            T mine = c;
#pragma unroll 8   // (unrolled whole, the 64 lane reads are hoisted and their scalar registers spill)
            for (int j = 0; j < kWave; j++) {
                if ((int)lane == j) mine = c;
                c = ordered_combine<OP>(c, wave_read_lane(t, j));
            }
            if (base + lane < rn) carry[rb + base + lane] = mine;
        }
    }
}

// ---- step 4: S = C (+) L in place, for the entries of the blocks b >= 1 -----------------------------------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(kCompactThreads) void scan_add_kernel(const int64_t *__restrict__ rowptr, const uint64_t *__restrict__ blkptr, uint64_t M,
                                                                   uint64_t nnz, const T *__restrict__ carry, T *__restrict__ out) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    const uint64_t last = (base + kCompactChunk < nnz ? base + kCompactChunk : nnz) - 1;
    // an entry's row as in chunk_entries_and_rows (osp_compact.h), without the columns
    const uint32_t r_first = (uint32_t)(upper_bound_dev(rowptr, 0, M + 1, (int64_t)base) - 1);
    const uint32_t r_last = (uint32_t)(upper_bound_dev(rowptr, (uint64_t)r_first + 1, M + 1, (int64_t)last) - 1);
    int64_t p[kCompactRounds];
    uint32_t lo[kCompactRounds], hi[kCompactRounds];
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        p[k] = (int64_t)(base + (uint64_t)k * kCompactThreads + threadIdx.x);
        lo[k] = r_first + 1;
        hi[k] = (uint64_t)p[k] < nnz ? r_last + 1 : r_first + 1;
    }
    if (r_first != r_last) bisect_together<true>(rowptr, lo, hi, p);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if ((uint64_t)p[k] >= nnz) continue;
        const uint32_t row = lo[k] - 1;
        const uint64_t q = (uint64_t)(p[k] - rowptr[row]);
        if (q >= kScanBlock) out[p[k]] = ordered_combine<OP>(carry[blkptr[row] + q / kScanBlock], out[p[k]]);
    }
}

// ---- the draw: cols[i s + d], pos[i s + d] for every row i and draw d --------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T draw_uniform(uint64_t h) {
    if constexpr (sizeof(T) == 8) return (T)(h >> 11) * 0x1p-53;
    else return (T)(uint32_t)(h >> 40) * 0x1p-24f;
}

// POS: the caller wants the positions as well (pos is not touched otherwise)
template <class T, bool POS>
__global__ __launch_bounds__(256) void draw_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, const T *__restrict__ cdf,
                                                   uint64_t total_draws, uint32_t s, uint64_t s0, int64_t *__restrict__ cols,
                                                   int64_t *__restrict__ pos) {
#pragma clang fp contract(off)
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < total_draws; x += (uint64_t)gridDim.x * 256) {
        const uint64_t i = x / s, d = x - i * s;
        const int64_t b = rowptr[i], e = rowptr[i + 1];
        int64_t at = -1, c = -1;
        if (e > b) {
            const T total = cdf[e - 1];
            if (total > T(0) && total < (T)__builtin_inf()) {
                const T t = draw_uniform<T>(select_k_mix(s0 ^ (i << 32 | d))) * total;
                // the first q with S_q > t || S_q == total; the row's last entry satisfies it
                int64_t lo = b, hi = e - 1;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    const T v = cdf[mid];
                    if (v > t || v == total) hi = mid; else lo = mid + 1;
                }
                at = lo;
                c = (int64_t)col[lo];
            }
        }
        cols[x] = c;
        if constexpr (POS) pos[x] = at;
    }
}

// out += the rows whose draws are -1 (for the stats: a workgroup's scan and one integer atomic each, as arg_count_kernel)
__global__ __launch_bounds__(256) void draw_without_kernel(const int64_t *__restrict__ cols, uint64_t M, uint32_t s, unsigned long long *__restrict__ out) {
    __shared__ uint64_t scratch[256 / kWave + 1];
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (uint64_t)gridDim.x * blockDim.x) sum += cols[i * s] < 0;
    uint64_t total;
    block_excl_scan<uint64_t, 256>(sum, scratch, &total);
    if (threadIdx.x == 0 && total) atomicAdd(out, (unsigned long long)total);
}

}  // namespace osp
