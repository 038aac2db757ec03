// osp_vector.h -- where a CSR result meets a dense per-vertex vector (osp_csr_reduce, osp_csr_apply_vectors,
// osp_csr_select_vertices, include/outerspace_spgemm_vector.h), written for gfx950 (wave64).  DESIGN.md section 14.
//
// Reduce.  The order of a segment's reduction R is part of the interface (wave_ordered_reduce, osp_prims.h: the order of
// osp_csr_inflate_prune's row sums) and depends on the segment's length alone, so the work may be cut freely:
//   * a segment of at most kReduceBlock entries is ONE wave's R, four waves to a workgroup (segments_short_kernel);
//   * a longer segment is cut into blocks of kReduceBlock: one wave per BLOCK writes r_b = R(block b) to a pool buffer
//     (segments_blocks_kernel), and the blocks' results of one segment are a segment of the next level, reduced by the same
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

// ---- the skeleton of R: three pieces, all template parameters (no branch on any of them in a kernel) -----------------------------
//   the accumulator, what a lane carries: PlainAcc (p), PairAcc (p and the winner's column, osp_mxv_arg.h).  It starts as the
//     identity, takes an entry of a source (take), another accumulator (combine) and hands out the one of the lane d above
//     (down); Acc::Stored is the array form of its kind;
//   the source, where entries come from: Values, Pairs (osp_mxv_arg.h), Products (osp_mxv.h).  value(i) is entry i's value; the
//     sources a PairAcc reads have column(i) and value(i, that column) as well;
//   the sink, where lane 0 stores: Values (out[i]; a level's partial results as well), Pairs (partial[i], pcol[i]) and ArgSink
//     (out[i], arg[i]; both osp_mxv_arg.h).
// DESIGN.md section 26 lists which operation runs which combination.

// stored values: a source, and the sink of plain accumulators
template <class T>
struct Values {
    T *vals;
    __device__ __forceinline__ T value(uint64_t i) const { return vals[i]; }
    template <class Acc>
    __device__ __forceinline__ void store(uint64_t i, const Acc &a) const {
        vals[i] = a.p;
    }
};

template <int OP, class T>
struct PlainAcc {
    typedef Values<T> Stored;
    T p = ordered_identity<OP, T>();
    __device__ __forceinline__ void combine(const PlainAcc &o) { p = ordered_combine<OP>(p, o.p); }
    // (asks the source for no column: Products then loads none under FIRST)
    template <class Src>
    __device__ __forceinline__ void take(const Src &src, uint64_t i) {
        combine(PlainAcc{src.value(i)});
    }
    __device__ __forceinline__ PlainAcc down(int d) const { return PlainAcc{__shfl_down(p, d, kWave)}; }
};

// the butterfly's steps d < below, the same in every lane (64: a whole wave; g: a packed row's g lanes, osp_mxv.h)
template <class Acc>
__device__ __forceinline__ void butterfly(Acc &a, uint32_t below) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1)
        if ((uint32_t)d < below) a.combine(a.down(d));
}

// R of the entries [b, b + m) of src by ONE wave, m <= kReduceBlock: wave_ordered_reduce (osp_prims.h) on any accumulator and
// source.  Lane 0 holds the result.
template <class Acc, class Src>
__device__ __forceinline__ Acc wave_reduce(const Src &src, uint64_t b, uint64_t m) {
    Acc a;
    for (uint64_t i = lane_id(); i < m; i += kWave) a.take(src, b + i);
    butterfly(a, kWave);
    return a;
}

// ---- segments of at most kReduceBlock entries, a wave each ------------------------------------------------------------------
// sink[map ? map[seg] : seg] = R(segment seg); longer segments are left to the block path
template <class Acc, class Src, class Sink>
__global__ __launch_bounds__(kReduceWaves *kWave) void segments_short_kernel(const int64_t *__restrict__ ptr, Src src, uint64_t nseg,
                                                                             const uint32_t *__restrict__ map, Sink sink) {
    const uint64_t seg = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const int64_t b = ptr[seg];
    const uint64_t m = (uint64_t)(ptr[seg + 1] - b);
    if (m > kReduceBlock) return;
    const Acc a = wave_reduce<Acc>(src, (uint64_t)b, m);
    if (lane_id() == 0) sink.store(map ? map[seg] : seg, a);
}

// ---- rows of at most kReduceBlock entries, packed: 64 >> lg consecutive rows per wave, g = 1 << lg lanes each when all of them
// fit (osp_mxv.h states why g lanes and log2(g) shuffles are the whole of R) ----------------------------------------------------
template <class Acc, class Src, class Sink>
__global__ __launch_bounds__(kReduceWaves *kWave) void segments_rows_kernel(const int64_t *__restrict__ rowptr, Src src, uint64_t M, uint32_t lg,
                                                                            Sink sink) {
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
        // (a lane past its row's entries holds the identity, which changes no accumulator it is combined into; a shuffle reaches
        // across a group's end only for lanes whose accumulator nobody uses)
        const uint32_t k = lane & (g - 1);
        Acc a;
        if (k < m) a.take(src, (uint64_t)b + k);
        butterfly(a, g);
        if (k == 0 && row < M) sink.store(row, a);
        return;
    }
    // a row of the batch does not fit its g lanes: the rows one after another, 64 lanes each
    for (uint32_t r = 0; r < (kWave >> lg) && r0 + r < M; r++) {
        const uint64_t rb = (uint64_t)__shfl((long long)b, (int)(r << lg), kWave), rm = (uint64_t)__shfl((long long)m, (int)(r << lg), kWave);
        if (rm > kReduceBlock) continue;   // (the block path writes it)
        const Acc a = wave_reduce<Acc>(src, rb, rm);
        if (lane == 0) sink.store(r0 + r, a);
    }
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
template <class Acc, class Src, class Sink>
__global__ __launch_bounds__(kReduceWaves *kWave) void segments_blocks_kernel(const int64_t *__restrict__ ptr, Src src,
                                                                              const uint32_t *__restrict__ long_segs, const int64_t *__restrict__ blkptr,
                                                                              uint64_t n_long, Sink partial) {
    const uint64_t w = (uint64_t)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
    if (w >= (uint64_t)blkptr[n_long]) return;   // (the grid covers the host's upper bound of the blocks)
    const uint64_t k = upper_bound_dev(blkptr, 0, n_long + 1, (int64_t)w) - 1;   // (same addresses in every lane)
    const uint32_t seg = long_segs[k];
    const uint64_t b = (uint64_t)ptr[seg] + (w - (uint64_t)blkptr[k]) * kReduceBlock, e = (uint64_t)ptr[seg + 1];
    const Acc a = wave_reduce<Acc>(src, b, e - b < kReduceBlock ? e - b : (uint64_t)kReduceBlock);
    if (lane_id() == 0) partial.store(w, a);
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
