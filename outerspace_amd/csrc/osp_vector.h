// osp_vector.h -- where a CSR result meets a dense per-vertex vector (osp_csr_reduce, osp_csr_apply_vectors,
// osp_csr_select_vertices, include/outerspace_spgemm_vector.h), written for gfx950 (wave64).  DESIGN.md section 14.
//
// Reduce.  The order of a segment's reduction R is part of the interface (wave_ordered_reduce, osp_prims.h: the order of
// osp_csr_inflate_prune's row sums) and depends on the segment's length alone, so the work may be cut freely:
//   * a segment of at most kReduceBlock entries is ONE wave's R, four waves to a workgroup (reduce_short_kernel);
//   * a longer segment is cut into blocks of kReduceBlock: one wave per BLOCK writes r_b = R(block b) to a pool buffer
//     (reduce_blocks_kernel), and the blocks' results of one segment are a segment of the next level, reduced by the same
//     two kernels until nothing is long (three levels reach 2^33 entries).  A frontier's one row of 2^20 entries is 512
//     waves, a product's 2^22 rows of a dozen are 2^22: neither is one workgroup's loop.
// Long segments are listed by mcl_classify_kernel (any order: every segment is handled on its own).  The column axis runs
// the same kernels on the column-major view (masked_view: one stable sort by column).  No float atomics, no waiting
// between workgroups: every output is a function of its inputs alone, the property osp_compact.h states.
//
// Apply.  Work is cut by entries.  The row side needs an entry's row (chunk_entries_and_rows); the column side is a stream
// over colidx with a gather of y.  One launch per side, the second in place on out's values: the operator is a template
// parameter (no branch on it in a kernel), values are moved as integers of their width.
//
// Vertex select.  One flag kernel, templated on which keep vectors are present, feeds osp_compact.h's three passes.
#pragma once
#include "osp_ewise.h"
#include "osp_mcl.h"

namespace osp {

constexpr uint32_t kReduceBlock = 2048;   // entries of one block of R: the longest segment one wave reduces
constexpr int kReduceWaves = 4;           // waves (segments or blocks) per workgroup
static_assert(kReduceBlock == kMclLongMin, "mcl_classify_kernel's threshold and R's block are one number in the documents");

// ---- reduce: segments of at most kReduceBlock entries, a wave each ---------------------------------------------------------
// out[map ? map[seg] : seg] = R(segment seg); longer segments are left to the block path
template <class T, int OP>
__global__ __launch_bounds__(kReduceWaves *kWave) void reduce_short_kernel(const int64_t *__restrict__ ptr, const T *__restrict__ vals, uint64_t nseg,
                                                                           const uint32_t *__restrict__ map, T *__restrict__ out) {
    const uint64_t seg = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const int64_t b = ptr[seg];
    const uint64_t m = (uint64_t)(ptr[seg + 1] - b);
    if (m > kReduceBlock) return;
    const T r = wave_ordered_reduce<OP>(vals + b, m);
    if (lane_id() == 0) out[map ? map[seg] : seg] = r;
}

// ---- reduce: what a level's long segments hand to the next level -----------------------------------------------------------
// nblk[k] = the blocks of long segment k, next_map[k] = where its result goes in the output vector
__global__ __launch_bounds__(256) void reduce_long_setup_kernel(const int64_t *__restrict__ ptr, const uint32_t *__restrict__ long_segs, uint64_t n_long,
                                                                const uint32_t *__restrict__ map, uint32_t *__restrict__ nblk,
                                                                uint32_t *__restrict__ next_map) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_long) return;
    const uint32_t seg = long_segs[k];
    nblk[k] = (uint32_t)(((uint64_t)(ptr[seg + 1] - ptr[seg]) + kReduceBlock - 1) / kReduceBlock);
    next_map[k] = map ? map[seg] : seg;
}

// partial[w] = R(block w): block w belongs to the long segment k with blkptr[k] <= w < blkptr[k + 1] and is that
// segment's block w - blkptr[k]; (blkptr, partial) are the next level's segments
template <class T, int OP>
__global__ __launch_bounds__(kReduceWaves *kWave) void reduce_blocks_kernel(const int64_t *__restrict__ ptr, const T *__restrict__ vals,
                                                                            const uint32_t *__restrict__ long_segs, const int64_t *__restrict__ blkptr,
                                                                            uint64_t n_long, T *__restrict__ partial) {
    const uint64_t w = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (w >= (uint64_t)blkptr[n_long]) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t k = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;   // (same addresses in every lane)
    const uint32_t seg = long_segs[k];
    const uint64_t b = (uint64_t)ptr[seg] + (w - (uint64_t)blkptr[k]) * kReduceBlock, e = (uint64_t)ptr[seg + 1];
    const T r = wave_ordered_reduce<OP>(vals + b, e - b < kReduceBlock ? e - b : (uint64_t)kReduceBlock);
    if (lane_id() == 0) partial[w] = r;
}

// ---- reduce, COUNT: out[seg] = (T)length; reads no value.  counter += segments longer than kReduceBlock ---------------------
template <class T>
__global__ __launch_bounds__(256) void reduce_count_kernel(const int64_t *__restrict__ ptr, uint64_t nseg, T *__restrict__ out,
                                                           unsigned long long *__restrict__ n_long) {
    const uint64_t seg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t m = 0;
    if (seg < nseg) {
        m = (uint64_t)(ptr[seg + 1] - ptr[seg]);
        out[seg] = (T)m;
    }
    const uint64_t longs = __ballot(m > kReduceBlock);
    if (longs && lane_id() == 0) atomicAdd(n_long, (unsigned long long)__popcll(longs));
}

// ---- apply: the row side, out[p] = op(src[p], x[row of p]) --------------------------------------------------------------------
// (src may be out itself: an entry is read and written by one lane)
template <class T, int OP>
__global__ __launch_bounds__(kCompactThreads) void apply_rows_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, uint64_t M,
                                                                     uint64_t nnz, const ValueBits<T> *src, const ValueBits<T> *__restrict__ x,
                                                                     ValueBits<T> *out) {
    typedef ValueBits<T> V;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        if ((uint64_t)p[k] >= nnz) continue;
        // (SECOND reads no value of src: the unused load is gone with the constant OP)
        out[p[k]] = ewise_apply<OP, T, V>(OP == EW_SECOND ? (V)0 : src[p[k]], x[lo[k] - 1]);
    }
}

// ---- apply: the column side, out[p] = op(src[p], y[col[p]]) --------------------------------------------------------------------
template <class T, int OP>
__global__ __launch_bounds__(256) void apply_cols_kernel(const uint32_t *__restrict__ col, uint64_t nnz, const ValueBits<T> *src,
                                                         const ValueBits<T> *__restrict__ y, ValueBits<T> *out) {
    typedef ValueBits<T> V;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    out[p] = ewise_apply<OP, T, V>(OP == EW_SECOND ? (V)0 : src[p], y[col[p]]);
}

// ---- vertex select, pass 1: keep_rows[row(p)] != 0 && keep_cols[col[p]] != 0, each side only when present ---------------------
template <bool ROWS, bool COLS>
__global__ __launch_bounds__(kCompactThreads) void vertex_flag_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, uint64_t M,
                                                                      uint64_t nnz, const uint8_t *__restrict__ keep_rows,
                                                                      const uint8_t *__restrict__ keep_cols, uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kCompactChunk;
    if (base >= nnz) return;
    uint32_t lo[kCompactRounds], hi[kCompactRounds], j[kCompactRounds];
    int64_t p[kCompactRounds];
    if constexpr (ROWS) {
        chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
    } else {
#pragma unroll
        for (int k = 0; k < kCompactRounds; k++) {
            p[k] = (int64_t)(base + (uint64_t)k * kCompactThreads + threadIdx.x);
            j[k] = (uint64_t)p[k] < nnz ? col[p[k]] : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < kCompactRounds; k++) {
        bool keep = (uint64_t)p[k] < nnz;
        if constexpr (ROWS) keep = keep && keep_rows[lo[k] - 1] != 0;
        if constexpr (COLS) keep = keep && keep_cols[j[k]] != 0;
        store_verdicts(keep, (uint64_t)p[k], nnz, bits);
    }
}

}  // namespace osp
