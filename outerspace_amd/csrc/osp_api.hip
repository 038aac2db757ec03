// osp_api.hip -- C ABI (include/outerspace_spgemm.h) and host orchestration of the GPU pipeline.
//
// Reference call stack being replaced:
//   parts = cscMulcsr(csc, csr)      SimSpGEMM.cpp:265-281   -> symbolic + multiply_kernel
//   C     = deduplicateCOO(concat)   SimSpGEMM.cpp:519-535   -> merge_tiles_kernel / global sort
// There is no CPU fallback here: every entry point needs a gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/outerspace_spgemm.h"
#include "../../include/outerspace_spgemm_masked.h"
#include "../../include/outerspace_spgemm_mcl.h"
#include "../../include/outerspace_spgemm_apply_mask.h"
#include "../../include/outerspace_spgemm_select.h"
#include "../../include/outerspace_spgemm_ewise.h"
#include "../../include/outerspace_spgemm_vector.h"
#include "../../include/outerspace_spgemm_mxm.h"
#include "../../include/outerspace_spgemm_transpose.h"
#include "../../include/outerspace_spgemm_mxv.h"
#include "../../include/outerspace_spgemm_extract.h"
#include "../../include/outerspace_spgemm_build.h"
#include "osp_internal.h"
#include "osp_kernels.h"
#include "osp_split.h"
#include "osp_sort.h"
#include "osp_epilogue.h"
#include "osp_conv.h"
#include "osp_masked.h"
#include "osp_mcl.h"
#include "osp_apply_mask.h"
#include "osp_select.h"
#include "osp_ewise.h"
#include "osp_vector.h"
#include "osp_mxm.h"
#include "osp_transpose.h"
#include "osp_mxv.h"
#include "osp_extract.h"
#include "osp_build.h"

namespace osp {

// (fail() and the per-thread error string live in osp_host.cpp, the host-only TU)

#define OSP_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            throw Error(e_ == hipErrorOutOfMemory ? OSP_ERR_ALLOC : OSP_ERR_HIP,           \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

#include "osp_context.h"
#include "osp_pipeline.h"

// Copies an input array to the device when it lives on the host.
template <class T>
static const T *to_device(Scratch &sc, const T *p, uint64_t n, osp_memspace_t space, hipStream_t s) {
    if (space == OSP_DEVICE || n == 0) return p;
    T *d = sc.get<T>(n);
    copy_h2d(d, p, n * sizeof(T), s);
    return d;
}

static void check_flags(uint32_t f, const char *what) {
    if (f & kFlagPtr) throw Error(OSP_ERR_ARG, std::string(what) + ": pointer array is not a monotone 0..nnz sequence");
    if (f & kFlagRange) throw Error(OSP_ERR_RANGE, std::string(what) + ": index outside its dimension");
    if (f & kFlagDuplicate) throw Error(OSP_ERR_DUPLICATE, std::string(what) + ": duplicate coordinate (reference: throw(233))");
    if (f & kFlagUnsorted) throw Error(OSP_ERR_UNSORTED, std::string(what) + ": indices inside a segment are not ascending");
}

// The end of a timed call: waits for its stream, then its time and every phase's time into the result (a phase the call
// never began reads 0).
static void finish_timing(Result *res, EventPair &ev, PhaseTimer &tm, hipStream_t s) {
    OSP_HIP(hipEventRecord(ev.b, s));
    OSP_HIP(hipStreamSynchronize(s));
    osp_result_info_t &i = res->info;
    i.ms_total = ev.ms();
    i.ms_symbolic = tm.total(PH_SYM);
    i.ms_multiply = tm.total(PH_MUL);
    i.ms_merge = tm.total(PH_MERGE);
    i.ms_compact = tm.total(PH_COMPACT);
    i.ms_multiply_kernel = tm.total(PH_MUL_K);
    i.ms_merge_kernel = tm.total(PH_MERGE_K);
    i.ms_split_kernel = tm.total(PH_SPLIT_K);
    i.ms_direct_plan_kernel = tm.total(PH_PLAN_K);
    i.ms_hub_plan_kernel = tm.total(PH_HUB_K);
    i.ms_expand_kernel = tm.total(PH_EXPAND_K);
}

// *out += sum_k nnz(A[:,k]) * nnz(B[k,:]) over all k (one atomic per workgroup)
__global__ void count_partials_kernel(const int64_t *a_colptr, const int64_t *b_rowptr, uint64_t K, unsigned long long *out) {
    __shared__ uint64_t scratch[256 / kWave + 1];
    uint64_t sum = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (uint64_t)gridDim.x * blockDim.x)
        sum += (uint64_t)(a_colptr[k + 1] - a_colptr[k]) * (uint64_t)(b_rowptr[k + 1] - b_rowptr[k]);
    uint64_t total;
    block_excl_scan<uint64_t, 256>(sum, scratch, &total);
    if (threadIdx.x == 0 && total) atomicAdd(out, (unsigned long long)total);
}

template <class T>
static void spgemm_impl(Context *ctx, Result *res, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr_in,
                        const uint32_t *a_rowidx_in, const T *a_vals_in, const int64_t *b_rowptr_in,
                        const uint32_t *b_colidx_in, const T *b_vals_in, osp_memspace_t space,
                        const osp_config_t &cfg, const PanelSink *sink = nullptr, bool partials_only = false) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    PhaseTimer tm(s);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    res->info.M = M; res->info.K = K; res->info.N = N;

    // pointer arrays first: nnz comes from their last entries
    const int64_t *a_colptr = to_device(sc, a_colptr_in, K + 1, space, s);
    const int64_t *b_rowptr = to_device(sc, b_rowptr_in, K + 1, space, s);
    int64_t nnz_a, nnz_b;
    // (with them comes the number of partial products of the whole product -- a sum over k of two differences: what decides
    // whether a product of few non-zeros still plans direct rows, see `direct` below)
    uint64_t p_all = 0;
    unsigned long long *p_all_dev = (unsigned long long *)sc.get<uint64_t>(1);
    zero_async(s, {{p_all_dev, sizeof(uint64_t)}});
    // (few workgroups: every one ends in an atomic on ONE word, 11-13 ns apiece -- 3 579 of them were the 46 us this kernel took
    // on the web-Google shape)
    if (K) count_partials_kernel<<<(unsigned)std::min<uint64_t>(grid_for(K, 256), 256), 256, 0, s>>>(a_colptr, b_rowptr, K, p_all_dev);
    {
        Gather g(s);
        if (space == OSP_HOST) { nnz_a = a_colptr_in[K]; nnz_b = b_rowptr_in[K]; }
        else { g.add(&nnz_a, a_colptr + K); g.add(&nnz_b, b_rowptr + K); }
        g.add(&p_all, (const uint64_t *)p_all_dev);
        g.wait();
    }
    if (nnz_a < 0 || nnz_b < 0) throw Error(OSP_ERR_ARG, "negative nnz in pointer array");
    if ((uint64_t)nnz_a >= 0xffffffffull || (uint64_t)nnz_b >= 0xffffffffull)
        throw Error(OSP_ERR_ARG, "operands with >= 2^32 non-zeros are not supported");
    const uint32_t *a_rowidx = to_device(sc, a_rowidx_in, nnz_a, space, s);
    const T *a_vals = to_device(sc, a_vals_in, nnz_a, space, s);
    const uint32_t *b_colidx = to_device(sc, b_colidx_in, nnz_b, space, s);
    const T *b_vals = to_device(sc, b_vals_in, nnz_b, space, s);
    res->info.nnz_a = nnz_a;
    res->info.nnz_b = nnz_b;

    if (cfg.validate) {
        uint32_t *flags = sc.get<uint32_t>(2);
        OSP_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), s));
        validate_ptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(a_colptr, K, nnz_a, flags);
        validate_ptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(b_rowptr, K, nnz_b, flags + 1);
        uint32_t fa = 0, fb = 0;
        { Gather g(s); g.add(&fa, (const uint32_t *)flags); g.add(&fb, (const uint32_t *)flags + 1); g.wait(); }
        check_flags(fa, "A (CSC)");
        check_flags(fb, "B (CSR)");
        if (nnz_a) validate_idx_kernel<<<grid_for(nnz_a, 256), 256, 0, s>>>(a_colptr, a_rowidx, K, nnz_a, M, flags);
        if (nnz_b) validate_idx_kernel<<<grid_for(nnz_b, 256), 256, 0, s>>>(b_rowptr, b_colidx, K, nnz_b, N, flags + 1);
        { Gather g(s); g.add(&fa, (const uint32_t *)flags); g.add(&fb, (const uint32_t *)flags + 1); g.wait(); }
        check_flags(fa, "A (CSC)");
        check_flags(fb, "B (CSR)");
    }

    // ---- k shard ----
    const uint64_t k0 = cfg.k_begin, k1 = cfg.k_end ? cfg.k_end : K;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] spgemm M=%llu K=%llu N=%llu nnzA=%lld nnzB=%lld k=[%llu,%llu) %s operands\n", (unsigned long long)M,
                (unsigned long long)K, (unsigned long long)N, (long long)nnz_a, (long long)nnz_b, (unsigned long long)k0,
                (unsigned long long)k1, space == OSP_HOST ? "host" : "device");
    if (k0 > k1 || k1 > K) throw Error(OSP_ERR_ARG, "k range outside [0,K]");
    int64_t e0 = 0, e1 = nnz_a;
    if (k0 != 0 || k1 != K) {
        if (space == OSP_HOST) { e0 = a_colptr_in[k0]; e1 = a_colptr_in[k1]; }
        else { Gather g(s); g.add(&e0, a_colptr + k0); g.add(&e1, a_colptr + k1); g.wait(); }
    }
    // ---- row-sharded multi-GPU mode: find this rank's rows and drop the rest of A BEFORE the symbolic phase ----
    // (a rank then sorts 1/G of A's non-zeros instead of all of them; every rank derives the same bounds from the
    // replicated operands alone: no collective)
    uint64_t r_lo = 0, r_hi = M;
    const bool row_sharded = cfg.row_shard_count > 1;
    if (row_sharded) {
        const uint64_t nnz = (uint64_t)(e1 - e0);  // all of the k shard's non-zeros: the pre-pass sees every row
        if (cfg.row_shard_index < 0 || cfg.row_shard_index >= cfg.row_shard_count) throw Error(OSP_ERR_ARG, "row shard index out of range");
        const uint32_t G = (uint32_t)cfg.row_shard_count;
        tm.begin(PH_SYM);
        {
            Scratch cs(ctx);
            unsigned long long *work = (unsigned long long *)cs.get<uint64_t>(M + 1);
            uint64_t *pre = cs.get<uint64_t>(M + 1), *cost_pre = cs.get<uint64_t>(M + 1);
            uint64_t *tmp = cs.get<uint64_t>(scan_scratch_entries(M + 1));
            uint64_t *d_b = cs.get<uint64_t>(2ull * (G + 1));
            OSP_HIP(hipMemsetAsync(work, 0, (M + 1) * sizeof(uint64_t), s));
            // every 16th column is sample enough to balance G shards of a large matrix; small ones are counted exactly
            const uint32_t stride = (k1 - k0) >= (1u << 16) ? 16u : 1u;
            const uint64_t nsample = (k1 - k0 + stride - 1) / stride;
            if (nnz) row_work_kernel<<<grid_for(nsample * kWave, 256), 256, 0, s>>>(a_colptr, a_rowidx, b_rowptr, k0, k1, stride, work);
            device_exclusive_scan<LoadU64, uint64_t>(LoadU64{(const uint64_t *)work}, M, pre, tmp, s);
            device_exclusive_scan<RowCost, uint64_t>(RowCost{pre, (uint64_t)TileCap<T>::value, kSplitRowMax}, M, cost_pre, tmp, s);
            shard_bounds_kernel<<<grid_for(G + 1, 64), 64, 0, s>>>(cost_pre, pre, M, G, d_b, d_b + G + 1);
            std::vector<uint64_t> h_b(2ull * (G + 1));
            copy_d2h(h_b.data(), d_b, h_b.size() * sizeof(uint64_t), s);
            r_lo = h_b[cfg.row_shard_index];
            r_hi = h_b[cfg.row_shard_index + 1];
        }
        // A restricted to rows [r_lo, r_hi): same K columns, absolute row ids
        int64_t *colptr2 = sc.get<int64_t>(K + 1);
        uint64_t nnz2 = 0;
        uint32_t *rowidx2 = nullptr;
        T *vals2 = nullptr;
        {
            Scratch cs(ctx);
            uint32_t *keep_scan = cs.get<uint32_t>(nnz + 1);
            uint32_t *tmp = cs.get<uint32_t>(scan_scratch_entries(nnz + 1));
            const RowInRange keep{a_rowidx + e0, (uint32_t)r_lo, r_hi};
            device_exclusive_scan<RowInRange, uint32_t>(keep, nnz, keep_scan, tmp, s);
            nnz2 = d2h(keep_scan + nnz, s);
            rowidx2 = sc.get<uint32_t>(nnz2);
            vals2 = sc.get<T>(nnz2);
            restrict_colptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(a_colptr, K, e0, nnz, keep_scan, colptr2);
            if (nnz2) restrict_compact_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(keep, keep_scan, nnz, a_vals + e0, rowidx2, vals2);
        }
        tm.end(PH_SYM);
        a_colptr = colptr2; a_rowidx = rowidx2; a_vals = vals2;
        e0 = 0;  // columns before k0 are empty now
        e1 = (int64_t)nnz2;
    }
    const uint64_t nnz = (uint64_t)(e1 - e0);  // non-zeros of A inside the shard

    // ---- symbolic: chunk offsets in (row, k) order ----
    tm.begin(PH_SYM);
    uint64_t *row_off = sc.get<uint64_t>(M + 1);
    uint64_t *chunk_off = sc.get<uint64_t>(nnz);
    uint64_t P = 0;
    // Row-wise variant (cfg.algorithm): rows of up to one tile of partial products are computed inside the tile kernel
    // from the chunk table; B's offsets must fit 32 bits for it (otherwise the outer-product path runs as usual)
    const int algo = cfg.algorithm;
    if (algo != OSP_ALGO_OUTER && algo != OSP_ALGO_ROWWISE) throw Error(OSP_ERR_ARG, "unknown algorithm");
    const bool rowwise = algo == OSP_ALGO_ROWWISE && nnz && (uint64_t)nnz_b < 0xffffffffull && nnz < 0xffffffffull && !partials_only;
    ChunkTable<T> ct{};
    // Long rows that one workgroup could split are written straight into their column ranges by the multiply phase
    // ("direct" rows, osp_split.h) when the operands allow 32-bit B offsets.  OSP_DIRECT=0 switches that off (every long
    // row is then split after the multiply, as the parts-merging entry points do), OSP_DIRECT_MAX=<partial products>
    // bounds the rows it applies to.
    // Small products keep the split: the plan costs a handful of launches and a read-back, which a product of a few
    // milliseconds does not earn back (web-Google shape: 2.3 ms with the split, 2.7 with direct rows).  OSP_DIRECT_MIN_NNZ
    // moves that boundary (the tests set it to 0, so that their small inputs take the direct path).
    const uint64_t direct_min_nnz = getenv("OSP_DIRECT_MIN_NNZ") ? strtoull(getenv("OSP_DIRECT_MIN_NNZ"), nullptr, 10) : ((getenv("OSP_GATHER") && atoi(getenv("OSP_GATHER")) == 0) ? (8ull << 20) : (2ull << 20));
    // ... unless its output rows are dense on average (at least 0.375 partial products per entry of the M x N result -- three times the
    // density from which a long row's column ranges are capped at the dense accumulators' width, plan_panel): such rows are
    // written in a few wide ranges, long runs, and summed without a sort -- 4096^2 with 880 entries per row (3.6 M non-zeros,
    // 3.2 G partial products) 44.4 -> 26.4 ms, Graph500 scale 14 ef 512 100 -> 79 ms.
    const bool dense_avg = (long double)p_all * 8.0L >= 3.0L * (long double)M * (long double)N;
    const bool direct = nnz && (nnz >= direct_min_nnz || dense_avg) && (uint64_t)nnz_b < 0xffffffffull && nnz < 0xffffffffull && !partials_only &&
                        !(getenv("OSP_DIRECT") && atoi(getenv("OSP_DIRECT")) == 0);
    const uint64_t direct_max = std::min<uint64_t>(getenv("OSP_DIRECT_MAX") ? strtoull(getenv("OSP_DIRECT_MAX"), nullptr, 10) : kSplitRowMax,
                                                   kDirectDenseMax);   // (the planner counts a row's products in 21 bits)
    // Gathered rows (osp_kernels.h): the merge kernel forms the partial products of planned long rows and of short rows itself,
    // from run descriptors; on unless OSP_GATHER=0 (debugging aid, A/B timing: every row is then written by the multiply, as
    // until round 4) or the row-wise variant runs (its tile kernel is another instantiation).  OSP_GATHER=1: long rows only.
    const int gather_env = getenv("OSP_GATHER") ? atoi(getenv("OSP_GATHER")) : 2;
    const bool gather_ok = nnz && !rowwise && !partials_only && (uint64_t)nnz_b < 0xffffffffull && nnz < 0xffffffffull;
    // (short rows: only where long rows are planned too -- a product of a few million non-zeros does not earn the tables back:
    // web-Google shape 2.09 -> 2.50 ms with them)
    const bool gather_short = gather_ok && gather_env >= 2 && direct;
    ShortRuns<T> srun{};
    DirectSrc dsrc{};
    uint32_t n_long_rows = 1;
    if (nnz == 0) {
        OSP_HIP(hipMemsetAsync(row_off, 0, (M + 1) * sizeof(uint64_t), s));
    } else {
        Scratch ss(ctx);
        Scratch &keep = (rowwise || direct || gather_short) ? sc : ss;  // the chunk table outlives the symbolic phase
        uint32_t *ka = ss.get<uint32_t>(nnz), *pa = ss.get<uint32_t>(nnz), *kb = ss.get<uint32_t>(nnz), *pb = ss.get<uint32_t>(nnz);
        uint32_t *rows_sorted = (gather_short ? keep : ss).template get<uint32_t>(nnz), *perm = keep.get<uint32_t>(nnz), *w_sorted = ss.get<uint32_t>(nnz);
        uint32_t *bs_sorted = (rowwise || direct || gather_short) ? keep.get<uint32_t>(nnz) : nullptr;
        uint32_t *rowfirst = keep.get<uint32_t>(M + 1);
        uint32_t *hist = ss.get<uint32_t>(rs_hist_entries(nnz));
        uint32_t *hist_tmp = ss.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nnz)));
        uint64_t *offs_sorted = keep.get<uint64_t>(nnz + 1);
        uint64_t *scan_tmp = ss.get<uint64_t>(scan_scratch_entries(std::max<uint64_t>(nnz, M + 1)));
        // (row, k) order of A's non-zeros; the last sort pass also looks up each chunk's length
        const bool table = rowwise || direct || gather_short;   // keep the chunk table: (length, B row) pairs in `w`
        // (gathered rows: the A values ride along, so that the run descriptors' makers read them in (row, k) order)
        const bool with_av = gather_ok && gather_env >= 1 && (direct || gather_short);
        T *av_sorted = with_av ? keep.get<T>(nnz) : nullptr;
        uint32_t *w = ss.get<uint32_t>(with_av ? 4 * nnz : table ? 2 * nnz : nnz);
        uint32_t *bs = table ? w : nullptr;
        sym_chunk_len_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(a_colptr, b_rowptr, k0, k1, e0, nnz, w, bs,
                                                                with_av ? reinterpret_cast<const uint32_t *>(a_vals) : nullptr, (uint32_t)(sizeof(T) / 4));
        SymEpilogue sym_ep{w, bs, rows_sorted, perm, w_sorted, bs_sorted};
        if (with_av) { sym_ep.av_sorted = av_sorted; sym_ep.vwords = (uint32_t)(sizeof(T) / 4); }
        device_sort_rows<SymEpilogue>(a_rowidx + e0, nnz, std::max(1, bits_for(M)), ka, pa, kb, pb, hist, hist_tmp, sym_ep, s, ctx->rank_atomic);
        device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{w_sorted}, nnz, offs_sorted, scan_tmp, s);
        sym_row_offsets_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rows_sorted, offs_sorted, nnz, M, row_off, rowfirst);
        const uint64_t rw_cap = (rowwise || gather_short) ? (uint64_t)TileCap<T>::value : 0ull;   // rows the multiply skips
        // (lazily where only rows written through cells would read them: DirectSrc::ensure_chunk_off)
        const bool expand_rows_on = gather_short && !(getenv("OSP_EXPAND_ROWS") && atoi(getenv("OSP_EXPAND_ROWS")) == 0);
        if (!expand_rows_on) sym_scatter_offsets_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(perm, offs_sorted, rows_sorted, row_off, rw_cap, nnz, chunk_off);
        // (the product proper reads P together with the size of the result, merge_pipeline: one stream round trip less)
        if (partials_only || rowwise || row_sharded) P = d2h(offs_sorted + nnz, s);
        else P = kPartialsOnDevice;
        if (direct) {
            dsrc = DirectSrc{rowfirst, offs_sorted, bs_sorted, perm, b_colidx, chunk_off, direct_max};
            dsrc.b_rowptr = b_rowptr; dsrc.K = K; dsrc.nnz_b = (uint64_t)nnz_b; dsrc.keep = &sc;
            // gathered rows (osp_kernels.h): on unless OSP_GATHER=0 (debugging aid, A/B timing: every direct row is then written
            // by the multiply, as until round 4) or the row-wise variant runs (its tile kernel is another instantiation)
            dsrc.gather = gather_ok && gather_env >= 1;
            dsrc.expand_rows = expand_rows_on;
            if (expand_rows_on) { dsrc.chunk_off_ready = false; dsrc.rows_sorted = rows_sorted; dsrc.row_off = row_off; dsrc.rw_cap = rw_cap; dsrc.nnz = nnz; }
            dsrc.a_vals = with_av ? (const void *)av_sorted : (const void *)(a_vals + e0); dsrc.av_in_order = with_av; dsrc.b_vals = b_vals;
            if (dsrc.gather) {
                dsrc.gstat = (unsigned long long *)sc.get<uint64_t>(3);
                zero_async(s, {{dsrc.gstat, 3 * sizeof(uint64_t)}});
            }
        }
        if (gather_short) {
            // the short rows' chunks as run descriptors, chunks without entries left out (once per product)
            const ShortRunFlag sf{offs_sorted};
            uint32_t *cidx = ss.get<uint32_t>(nnz + 1), *cidx_tmp = ss.get<uint32_t>(scan_scratch_entries(nnz + 1));
            device_exclusive_scan<ShortRunFlag, uint32_t>(sf, nnz, cidx, cidx_tmp, s);
            RunDesc<T> *runs0 = sc.get<RunDesc<T>>(nnz);   // (bound: every chunk; the count stays on the device)
            uint32_t *rowfirst0 = sc.get<uint32_t>(M + 1);
            short_runs_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(sf, cidx, nnz, bs_sorted, av_sorted, runs0);
            short_rowfirst_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rowfirst, cidx, M, rowfirst0);
            srun = ShortRuns<T>{runs0, rowfirst0, b_colidx, b_vals};
        }
        if (rowwise) {
            ct = ChunkTable<T>{offs_sorted, bs_sorted, perm, rowfirst, a_vals + e0, b_colidx, b_vals, (uint32_t)rw_cap, 1u};
            uint32_t *flag_scan = ss.get<uint32_t>(M + 1);
            device_exclusive_scan<HeavyRowFlag, uint32_t>(HeavyRowFlag{row_off, 0, (uint32_t)rw_cap}, M, flag_scan, (uint32_t *)scan_tmp, s);
            n_long_rows = d2h(flag_scan + M, s);
        }
    }
    tm.end(PH_SYM);
    res->info.partials = P;

    OuterProducer<T> prod;
    prod.ctx = ctx; prod.res = res;
    prod.a_colptr = a_colptr; prod.a_rowidx = a_rowidx; prod.a_vals = a_vals;
    prod.b_rowptr = b_rowptr; prod.b_colidx = b_colidx; prod.b_vals = b_vals;
    prod.k0 = k0; prod.k1 = k1; prod.e0 = e0; prod.chunk_off = chunk_off;
    const uint64_t nk = k1 - k0;
    prod.a_start = sc.get<int64_t>(nk); prod.a_cnt = sc.get<uint32_t>(nk);
    prod.prod = sc.get<uint64_t>(nk); prod.prod_off = sc.get<uint64_t>(nk + 1);
    prod.scan_tmp = sc.get<uint64_t>(scan_scratch_entries(nk));
    prod.nothing_staged = rowwise && n_long_rows == 0;
    prod.short_gathered = gather_short;
    if ((dsrc.gather || gather_short) && nnz && !partials_only) {
        prod.nnz = nnz;
        prod.kscan = sc.get<uint32_t>(nnz + 1);
        prod.kscan_tmp = sc.get<uint32_t>(scan_scratch_entries(std::max<uint64_t>(nnz, k1 - k0) + 1));
        prod.elist = sc.get<uint32_t>(nnz);
        prod.cscan = sc.get<uint32_t>(k1 - k0 + 1);
        prod.klist = sc.get<uint32_t>(k1 - k0 + 1);
    }

    if (partials_only) {
        // osp_spgemm_partials: the multiply phase alone; offsets and records belong to the result
        if (row_sharded) throw Error(OSP_ERR_ARG, "partial products of a row shard are not supported");
        res->partials = true;
        res->rowptr = (int64_t *)ctx->alloc((M + 1) * sizeof(int64_t));
        OSP_HIP(hipMemcpyAsync(res->rowptr, row_off, (M + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
        res->vals = ctx->alloc(std::max<uint64_t>(P, 1) * sizeof(Part<T>));
        res->info.panels = 1;
        res->info.nnz_c = P;
        res->info.row_begin = 0;
        res->info.row_end = M;
        tm.begin(PH_MUL);
        if (P) prod.produce(0, M, true, 0, P, (Part<T> *)res->vals, tm, nullptr, nullptr);
        tm.end(PH_MUL);
        finish_timing(res, ev, tm, s);
        return;
    }
    // row-sharded: A holds this rank's rows only, so the staging offsets start at 0 at r_lo and P is the shard's count
    const uint64_t off_lo = 0, P_rows = P;
    merge_pipeline<T>(ctx, res, prod, M, N, row_off, P_rows, cfg.partial_capacity, tm, r_lo, r_hi, off_lo, sink,
                      rowwise ? &ct : nullptr, (direct && nnz) ? &dsrc : nullptr, nullptr, gather_short ? &srun : nullptr);

    finish_timing(res, ev, tm, s);
    if (gather_short) res->info.gathered_short_partials = res->info.partials - res->info.heavy_partials;
    if (dsrc.gstat && res->info.direct_rows) {
        uint64_t gs[3] = {0, 0, 0};
        copy_d2h(gs, dsrc.gstat, sizeof(gs), s);
        res->info.gathered_rows = gs[0]; res->info.gathered_partials = gs[1]; res->info.gathered_runs = gs[2];
    }
    if (getenv("OSP_VERBOSE")) {
        fprintf(stderr, "[osp] product done in %.1f ms; pool misses so far: %llu hipMalloc calls, %.1f GB, %.1f ms\n", res->info.ms_total,
                (unsigned long long)ctx->malloc_calls, ctx->malloc_bytes / 1e9, ctx->malloc_ms);
    }
}

// COO (device arrays, any order) -> compressed by `seg` with ascending `inner` indices; all outputs in `sc`.
template <class T>
static void coo_to_compressed_device(Context *ctx, Scratch &sc, uint64_t nseg, uint64_t ninner, uint64_t nnz, const uint32_t *seg,
                                     const uint32_t *inner, const T *vals, const char *what, int64_t **ptr_out,
                                     uint32_t **idx_out, T **val_out) {
    hipStream_t s = ctx->stream;
    int64_t *ptr = sc.get<int64_t>(nseg + 1);
    uint32_t *idx = sc.get<uint32_t>(nnz);
    T *ov = sc.get<T>(nnz);
    *ptr_out = ptr; *idx_out = idx; *val_out = ov;
    if (nnz == 0) {
        OSP_HIP(hipMemsetAsync(ptr, 0, (nseg + 1) * sizeof(int64_t), s));
        return;
    }
    Scratch ss(ctx);
    uint32_t *ka = ss.get<uint32_t>(nnz), *pa = ss.get<uint32_t>(nnz), *kb = ss.get<uint32_t>(nnz), *pb = ss.get<uint32_t>(nnz);
    uint32_t *k1 = ss.get<uint32_t>(nnz), *perm1 = ss.get<uint32_t>(nnz), *k2 = ss.get<uint32_t>(nnz);
    uint32_t *seg_sorted = ss.get<uint32_t>(nnz), *perm2 = ss.get<uint32_t>(nnz);
    uint32_t *hist = ss.get<uint32_t>(rs_hist_entries(nnz));
    uint32_t *hist_tmp = ss.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nnz)));
    uint32_t *flags = ss.get<uint32_t>(1);
    OSP_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
    // stable LSD: by inner index first, then by segment
    device_sort_rows<RsStoreEpilogue>(inner, nnz, std::max(1, bits_for(ninner)), ka, pa, kb, pb, hist, hist_tmp,
                                      RsStoreEpilogue{k1, perm1}, s, ctx->rank_atomic);
    ingest_gather_u32_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(seg, perm1, nnz, k2);
    device_sort_rows<RsStoreEpilogue>(k2, nnz, std::max(1, bits_for(nseg)), ka, pa, kb, pb, hist, hist_tmp,
                                      RsStoreEpilogue{seg_sorted, perm2}, s, ctx->rank_atomic, perm1);
    ingest_finish_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(seg_sorted, perm2, inner, vals, nnz, nseg, ninner, idx, ov, flags);
    ingest_ptr_kernel<<<grid_for(nseg + 1, 256), 256, 0, s>>>(seg_sorted, nnz, nseg, ptr);
    check_flags(d2h(flags, s), what);
}

template <class T>
static void spgemm_coo_impl(Context *ctx, Result *res, uint64_t M, uint64_t K, uint64_t N, uint64_t nnz_a, const uint32_t *a_rows,
                            const uint32_t *a_cols, const T *a_vals, uint64_t nnz_b, const uint32_t *b_rows, const uint32_t *b_cols,
                            const T *b_vals, osp_memspace_t space, const osp_config_t &cfg) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint32_t *ar = to_device(sc, a_rows, nnz_a, space, s), *ac = to_device(sc, a_cols, nnz_a, space, s);
    const uint32_t *br = to_device(sc, b_rows, nnz_b, space, s), *bc = to_device(sc, b_cols, nnz_b, space, s);
    const T *av = to_device(sc, a_vals, nnz_a, space, s), *bv = to_device(sc, b_vals, nnz_b, space, s);
    int64_t *ap, *bp;
    uint32_t *ai, *bi;
    T *acv, *bcv;
    coo_to_compressed_device<T>(ctx, sc, K, M, nnz_a, ac, ar, av, "A (COO)", &ap, &ai, &acv);  // csc = coo2csr<true>(A, K)
    coo_to_compressed_device<T>(ctx, sc, K, N, nnz_b, br, bc, bv, "B (COO)", &bp, &bi, &bcv);  // csr = coo2csr(B, K)
    OSP_HIP(hipEventRecord(ev.b, s));
    osp_config_t c2 = cfg;
    c2.validate = 0;  // ordering, ranges and duplicates were just established
    spgemm_impl<T>(ctx, res, M, K, N, ap, ai, acv, bp, bi, bcv, OSP_DEVICE, c2);
    const float ms = ev.ms();
    res->info.ms_ingest = ms;
    res->info.ms_total += ms;
}

// The reference's in-memory operands as they stand (osp_spgemm_csc_csr_aos): packed {u32 idx; T val} records -- the
// layout of Part<T> -- are split into index and value arrays on the device.
template <class T>
__global__ void aos_unpack_kernel(const Part<T> *__restrict__ data, uint64_t n, uint32_t *__restrict__ idx, T *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PartWords<T> r = load_part_words(data + i);
    idx[i] = r.col();
    val[i] = r.val();
}
template <class T>
static void spgemm_aos_impl(Context *ctx, Result *res, uint64_t M, uint64_t K, uint64_t N, const uint64_t *a_pos, const void *a_data,
                            const uint64_t *b_pos, const void *b_data, osp_memspace_t space, const osp_config_t &cfg) {
    static_assert(sizeof(Part<T>) == 4 + sizeof(T), "Part<T> must be the reference's packed CSRElement (common.h:10-16)");
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    // size_t offsets are taken as int64 (same bits below 2^63; larger values fail the pointer check)
    const int64_t *ap = to_device(sc, (const int64_t *)a_pos, K + 1, space, s);
    const int64_t *bp = to_device(sc, (const int64_t *)b_pos, K + 1, space, s);
    int64_t nnz_a, nnz_b;
    if (space == OSP_HOST) { nnz_a = (int64_t)a_pos[K]; nnz_b = (int64_t)b_pos[K]; }
    else { nnz_a = d2h(ap + K, s); nnz_b = d2h(bp + K, s); }
    if (nnz_a < 0 || nnz_b < 0 || (uint64_t)nnz_a >= 0xffffffffull || (uint64_t)nnz_b >= 0xffffffffull)
        throw Error(OSP_ERR_ARG, "operands with >= 2^32 non-zeros are not supported");
    if ((nnz_a && !a_data) || (nnz_b && !b_data)) throw Error(OSP_ERR_ARG, "null data array");
    const Part<T> *ad = to_device(sc, (const Part<T> *)a_data, (uint64_t)nnz_a, space, s);
    const Part<T> *bd = to_device(sc, (const Part<T> *)b_data, (uint64_t)nnz_b, space, s);
    uint32_t *ai = sc.get<uint32_t>(nnz_a), *bi = sc.get<uint32_t>(nnz_b);
    T *av = sc.get<T>(nnz_a), *bv = sc.get<T>(nnz_b);
    if (nnz_a) aos_unpack_kernel<T><<<grid_for(nnz_a, 256), 256, 0, s>>>(ad, (uint64_t)nnz_a, ai, av);
    if (nnz_b) aos_unpack_kernel<T><<<grid_for(nnz_b, 256), 256, 0, s>>>(bd, (uint64_t)nnz_b, bi, bv);
    spgemm_impl<T>(ctx, res, M, K, N, ap, ai, av, bp, bi, bv, OSP_DEVICE, cfg);
}

// The symbolic phase of a parts merge: the candidate chunks -- chunk (r, p) = row r of part p -- scanned into every row's
// offset into the staging (prod.row_off); info.partials = P, the entries of all parts.  `prod` reads the parts' rows
// through d_rp, the device array of their row pointers.
template <class Producer>
static void parts_symbolic(Context *ctx, Scratch &sc, PhaseTimer &tm, Result *res, const int64_t *const *d_rp, int nparts, uint64_t M,
                           Producer &prod) {
    hipStream_t s = ctx->stream;
    tm.begin(PH_SYM);
    const uint64_t ncand = M * (uint64_t)nparts;
    uint64_t *row_off = sc.get<uint64_t>(M + 1);
    uint64_t *offs = sc.get<uint64_t>(ncand + 1);
    uint64_t *scan_tmp = sc.get<uint64_t>(scan_scratch_entries(ncand));
    device_exclusive_scan<PartsChunkLen, uint64_t>(PartsChunkLen{d_rp, nparts}, ncand, offs, scan_tmp, s);
    parts_rows_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(offs, nparts, M, row_off);
    const uint64_t P = d2h(offs + ncand, s);
    tm.end(PH_SYM);
    res->info.partials = P;
    prod.ctx = ctx; prod.d_rowptrs = d_rp; prod.nparts = nparts; prod.row_off = row_off;
}

template <class T>
static void merge_parts_impl(Context *ctx, Result *res, uint64_t M, uint64_t N, int nparts,
                             const int64_t *const *rowptrs, const uint32_t *const *colidxs, const void *const *valss,
                             osp_memspace_t space, const osp_config_t &cfg) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    PhaseTimer tm(s);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    res->info.M = M; res->info.N = N;
    std::vector<const int64_t *> rp(nparts);
    std::vector<const uint32_t *> ci(nparts);
    std::vector<const T *> va(nparts);
    uint64_t nnz_in = 0;
    for (int p = 0; p < nparts; p++) {
        rp[p] = to_device(sc, rowptrs[p], M + 1, space, s);
        int64_t nnz = (space == OSP_HOST) ? rowptrs[p][M] : d2h(rp[p] + M, s);
        if (nnz < 0) throw Error(OSP_ERR_ARG, "negative nnz in part");
        ci[p] = to_device(sc, colidxs[p], nnz, space, s);
        va[p] = to_device(sc, (const T *)valss[p], nnz, space, s);
        nnz_in += nnz;
    }
    res->info.nnz_a = nnz_in;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] merge_csr_parts M=%llu N=%llu parts=%d entries=%llu %s operands\n", (unsigned long long)M,
                (unsigned long long)N, nparts, (unsigned long long)nnz_in, space == OSP_HOST ? "host" : "device");
    const int64_t **d_rp = (const int64_t **)sc.get<void *>(nparts);
    const uint32_t **d_ci = (const uint32_t **)sc.get<void *>(nparts);
    const T **d_va = (const T **)sc.get<void *>(nparts);
    copy_h2d(d_rp, rp.data(), nparts * sizeof(void *), s);
    copy_h2d(d_ci, ci.data(), nparts * sizeof(void *), s);
    copy_h2d(d_va, va.data(), nparts * sizeof(void *), s);
    PartsProducer<T> prod;
    prod.d_colidxs = d_ci; prod.d_valss = d_va;
    parts_symbolic(ctx, sc, tm, res, d_rp, nparts, M, prod);
    merge_pipeline<T>(ctx, res, prod, M, N, prod.row_off, res->info.partials, cfg.partial_capacity, tm);
    finish_timing(res, ev, tm, s);
}

template <class T>
static void merge_record_parts_impl(Context *ctx, Result *res, uint64_t M, uint64_t N, int nparts, const int64_t *const *rowptrs,
                                    const void *const *records, osp_memspace_t space, const osp_config_t &cfg,
                                    const std::vector<uint64_t> *cuts = nullptr,
                                    const std::function<void(uint64_t, uint64_t)> *before = nullptr) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    PhaseTimer tm(s);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    res->info.M = M; res->info.N = N;
    std::vector<const int64_t *> rp(nparts);
    std::vector<const Part<T> *> rc(nparts);
    uint64_t nnz_in = 0;
    for (int p = 0; p < nparts; p++) {
        rp[p] = to_device(sc, rowptrs[p], M + 1, space, s);
        const int64_t n = (space == OSP_HOST) ? rowptrs[p][M] : d2h(rp[p] + M, s);
        if (n < 0) throw Error(OSP_ERR_ARG, "negative record count in part");
        rc[p] = to_device(sc, (const Part<T> *)records[p], (uint64_t)n, space, s);
        nnz_in += (uint64_t)n;
    }
    res->info.nnz_a = nnz_in;
    if (cfg.validate) {
        // offsets monotone from 0 to the record count, columns below N: what the split and dense paths index with
        uint32_t *flags = sc.get<uint32_t>(1);
        OSP_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
        for (int p = 0; p < nparts; p++) {
            const uint64_t n = (uint64_t)((space == OSP_HOST) ? rowptrs[p][M] : d2h(rp[p] + M, s));
            validate_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rp[p], M, n, flags);
            if (n) validate_record_cols_kernel<T><<<grid_for(n, 256), 256, 0, s>>>(rc[p], n, N, flags);
        }
        check_flags(d2h(flags, s), "record parts");
    }
    const int64_t **d_rp = (const int64_t **)sc.get<void *>(nparts);
    const Part<T> **d_rc = (const Part<T> **)sc.get<void *>(nparts);
    copy_h2d(d_rp, rp.data(), nparts * sizeof(void *), s);
    copy_h2d(d_rc, rc.data(), nparts * sizeof(void *), s);
    RecordPartsProducer<T> prod;
    prod.d_recs = d_rc; prod.before = before;
    parts_symbolic(ctx, sc, tm, res, d_rp, nparts, M, prod);
    merge_pipeline<T>(ctx, res, prod, M, N, prod.row_off, res->info.partials, cfg.partial_capacity, tm, 0, ~0ull, 0, nullptr, nullptr,
                      nullptr, cuts);
    finish_timing(res, ev, tm, s);
}

// which of the two exact variants of the order-sensitive steps this context runs (visible in every result)
static void note_variants(const Context *ctx, Result *res) {
    res->info.rank_atomic = ctx->rank_atomic ? 1u : 0u;
    res->info.dense_atomic = ctx->dense_atomic[res->dtype == OSP_F64] ? 1u : 0u;
}

// ---- what the operations that make a CSR result from a CSR result share ----
static void alloc_rowptr(Result *res, uint64_t M) { res->rowptr = (int64_t *)res->ctx->alloc((M + 1) * sizeof(int64_t)); }
// (an empty result has arrays of one entry: its pointers are never null)
template <class T>
static void alloc_entries(Result *res, uint64_t nnz) {
    res->colidx = (uint32_t *)res->ctx->alloc(std::max<uint64_t>(nnz, 1) * sizeof(uint32_t));
    res->vals = res->ctx->alloc(std::max<uint64_t>(nnz, 1) * sizeof(T));
}
// the result of M rows without entries
template <class T>
static void empty_result(Result *res, uint64_t M, hipStream_t s) {
    alloc_rowptr(res, M);
    OSP_HIP(hipMemsetAsync(res->rowptr, 0, (M + 1) * sizeof(int64_t), s));
    alloc_entries<T>(res, 0);
}
// The end of such a call: waits for its stream, then the result's size and the call's time.
static void finish_csr(Result *res, EventPair &ev, uint64_t nnz, hipStream_t s) {
    OSP_HIP(hipEventRecord(ev.b, s));
    OSP_HIP(hipStreamSynchronize(s));
    OSP_HIP(hipGetLastError());
    res->info.nnz_c = nnz;
    res->info.ms_total = ev.ms();
}
// The two passes of an operation that works row by row on M rows: count(cnt) launches what writes the entries each row
// keeps to cnt[0..M), the scan of the counts is the result's row pointer, one read-back sizes the result, and write()
// launches what fills it (not when it is empty).  Returns the result's nnz.
template <class T, class Count, class Write>
static uint64_t rows_two_pass(Scratch &sc, Result *res, uint64_t M, hipStream_t s, Count &&count, Write &&write) {
    alloc_rowptr(res, M);
    uint32_t *cnt = sc.get<uint32_t>(M + 1);
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(M + 1));
    count(cnt);
    device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{cnt}, M, (uint64_t *)res->rowptr, tmp, s);
    const uint64_t nnz = (uint64_t)d2h(res->rowptr + M, s);
    alloc_entries<T>(res, nnz);
    if (nnz) write();
    return nnz;
}
// The first two passes of osp_compact.h over `n` (> 0) entries: flag(nchunks, bits) launches the flag kernel, then the scan of
// the words' popcounts and the call's ONE read-back (the number of set bits, and whatever `more` adds to it).
struct BitScan { uint64_t *bits, *pos; uint64_t count; uint32_t launches; };
template <class Flag>
static BitScan flag_and_scan(Scratch &sc, uint64_t n, hipStream_t s, Flag &&flag, const std::function<void(Gather &)> &more = nullptr) {
    const uint64_t nwords = (n + 63) / 64;
    BitScan b{sc.get<uint64_t>(nwords), sc.get<uint64_t>(nwords + 1), 0, 0};
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(nwords));
    flag(grid_for(n, (unsigned)kCompactChunk), b.bits);
    b.launches = 1 + device_exclusive_scan<LoadPopc64, uint64_t>(LoadPopc64{b.bits}, nwords, b.pos, tmp, s);
    Gather g(s);
    g.add(&b.count, (const uint64_t *)b.pos + nwords);
    if (more) more(g);
    g.wait();
    return b;
}
// The compaction of `in` by one verdict bit per entry (osp_compact.h): flag_and_scan, then the result at its exact size, its
// row pointer and its entries; with `fill` every kept entry gets that value and `in`'s values are not read.  An empty `in`
// launches nothing.
struct Compacted { uint64_t nnz; uint32_t launches; };
template <class T, class Flag>
static Compacted compact_by_bits(Scratch &sc, const Result *in, Result *res, hipStream_t s, Flag &&flag, const T *fill = nullptr,
                                 const std::function<void(Gather &)> &more = nullptr) {
    typedef typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type V;
    const uint64_t M = in->info.M, nnz_in = in->info.nnz_c;
    if (nnz_in == 0) {
        empty_result<T>(res, M, s);
        return {0, 0};
    }
    alloc_rowptr(res, M);
    const BitScan b = flag_and_scan(sc, nnz_in, s, flag, more);
    const uint64_t nnz = b.count;
    uint32_t launches = b.launches;
    alloc_entries<T>(res, nnz);
    compact_rowptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(in->rowptr, M, b.bits, b.pos, res->rowptr);
    launches++;
    if (nnz) {
        V fill_bits = 0;
        if (fill) memcpy(&fill_bits, fill, sizeof fill_bits);
        const auto write = fill ? compact_write_kernel<V, true> : compact_write_kernel<V, false>;
        write<<<grid_for(nnz_in, 256), 256, 0, s>>>(in->colidx, (const V *)in->vals, nnz_in, b.bits, b.pos, fill_bits, res->colidx, (V *)res->vals);
        launches++;
    }
    return {nnz, launches};
}

// relu(C + bias) with the zeros dropped, as a new CSR (osp_epilogue.h)
template <class T>
static void bias_relu_impl(Context *ctx, const Result *in, Result *res, const T *bias_in, osp_memspace_t bias_space, int relu) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N;
    const T *bias = bias_in ? to_device(sc, bias_in, N, bias_space, s) : nullptr;
    res->info = in->info;
    const unsigned grid = grid_for(std::max<uint64_t>(M, 1) * kWave, 256);
    const uint64_t nnz = rows_two_pass<T>(
        sc, res, M, s,
        [&](uint32_t *cnt) {
            bias_relu_rows_kernel<T, false><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, (const T *)in->vals, M, N, bias, relu, cnt, nullptr, nullptr,
                                                                 nullptr);
        },
        [&] {
            bias_relu_rows_kernel<T, true><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, (const T *)in->vals, M, N, bias, relu, nullptr, res->rowptr,
                                                                res->colidx, (T *)res->vals);
        });
    finish_csr(res, ev, nnz, s);
}

// ---- the conv stage of a sparse LeNet (osp_conv.h) ----
// The checks every conv entry point shares: the output size per axis, and every index of A and of the input within u32.
static ConvGeom conv_geometry(uint64_t N, uint64_t C, uint64_t H, uint64_t W, const osp_conv2d_geometry_t *geom) {
    if (!geom) throw Error(OSP_ERR_ARG, "null geometry");
    for (uint32_t r : geom->reserved)
        if (r) throw Error(OSP_ERR_ARG, "geometry: reserved fields must be zero");
    if (!N || !C || !H || !W) throw Error(OSP_ERR_ARG, "N, C, H and W must be >= 1");
    if (!geom->kh || !geom->kw || !geom->stride_h || !geom->stride_w || !geom->dil_h || !geom->dil_w)
        throw Error(OSP_ERR_ARG, "geometry: kernel, stride and dilation must be >= 1");
    const uint64_t lim = 0xffffffffull;
    if (C >= lim || H >= lim || W >= lim || (unsigned __int128)N * H * W >= lim)
        throw Error(OSP_ERR_RANGE, "N*H*W or C does not fit the u32 index type");
    const uint64_t eh = (uint64_t)geom->dil_h * (geom->kh - 1) + 1, ew = (uint64_t)geom->dil_w * (geom->kw - 1) + 1;
    const uint64_t hp = H + 2ull * geom->pad_h, wp = W + 2ull * geom->pad_w;
    if (hp < eh || wp < ew) throw Error(OSP_ERR_ARG, "geometry: the (dilated) kernel is larger than the padded input: empty output");
    const uint64_t OH = (hp - eh) / geom->stride_h + 1, OW = (wp - ew) / geom->stride_w + 1;
    if ((unsigned __int128)N * OH * OW >= lim) throw Error(OSP_ERR_RANGE, "N*OH*OW does not fit the u32 index type");
    if ((uint64_t)C * geom->kh * geom->kw >= lim) throw Error(OSP_ERR_RANGE, "C*kh*kw does not fit the u32 index type");
    return ConvGeom{(uint32_t)H, (uint32_t)W, geom->kh, geom->kw, geom->stride_h, geom->stride_w, geom->pad_h, geom->pad_w,
                    geom->dil_h, geom->dil_w, (uint32_t)OH, (uint32_t)OW};
}

// A = im2col(x) in CSC, x as device COO.  Returns nnz(A); with `fill`, writes A to colptr / rowidx / vals (allocated in
// `sc` when colptr is null on entry).  x is grouped by channel with the COO ingest (this also checks its ranges and
// duplicates), then units (column k, chunk of channel c) are counted, scanned in column-major order and written.
template <class T>
static uint64_t im2col_impl(Context *ctx, Scratch &sc, uint64_t N, uint64_t C, const ConvGeom &g, uint64_t nnz_x, const uint32_t *xr,
                            const uint32_t *xc, const T *xv, bool fill, int64_t *&colptr, uint32_t *&rowidx, T *&vals) {
    hipStream_t s = ctx->stream;
    const uint32_t khkw = g.kh * g.kw;
    const uint64_t K = C * khkw;
    int64_t *xptr;
    uint32_t *xpix;
    T *xval;
    coo_to_compressed_device<T>(ctx, sc, C, N * g.H * g.W, nnz_x, xc, xr, xv, "x (COO)", &xptr, &xpix, &xval);
    // units per channel: a few host words (C + 1), the one round trip of the layout
    std::vector<int64_t> hp(C + 1);
    copy_d2h(hp.data(), xptr, (C + 1) * sizeof(int64_t), s);
    std::vector<uint64_t> ub(C + 1);
    ub[0] = 0;
    for (uint64_t c = 0; c < C; c++) ub[c + 1] = ub[c] + (uint64_t)((hp[c + 1] - hp[c] + kConvChunk - 1) / kConvChunk) * khkw;
    const uint64_t U = ub[C];
    uint64_t *ubase = sc.get<uint64_t>(C + 1);
    copy_h2d(ubase, ub.data(), (C + 1) * sizeof(uint64_t), s);
    uint32_t *cnt = sc.get<uint32_t>(U);
    uint64_t *off = sc.get<uint64_t>(U + 1);
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(U + 1));
    const unsigned grid = grid_for(std::max<uint64_t>(U, 1) * kWave, 256);
    if (U)
        im2col_units_kernel<T, false><<<grid, 256, 0, s>>>(xptr, xpix, xval, ubase, (uint32_t)C, g, U, cnt, nullptr, nullptr, nullptr);
    device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{cnt}, U, off, tmp, s);
    const uint64_t nnz = d2h(off + U, s);
    if (!fill) return nnz;
    if (!colptr) {
        colptr = sc.get<int64_t>(K + 1);
        rowidx = sc.get<uint32_t>(nnz);
        vals = sc.get<T>(nnz);
    } else if (nnz && (!rowidx || !vals)) {
        throw Error(OSP_ERR_ARG, "null a_rowidx or a_vals for a non-empty A");
    }
    im2col_colptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(ubase, off, (uint32_t)C, khkw, U, colptr);
    if (nnz) im2col_units_kernel<T, true><<<grid, 256, 0, s>>>(xptr, xpix, xval, ubase, (uint32_t)C, g, U, nullptr, off, rowidx, vals);
    OSP_HIP(hipStreamSynchronize(s));
    OSP_HIP(hipGetLastError());
    return nnz;
}

template <class T>
static void spgemm_conv2d_impl(Context *ctx, Result *res, uint64_t N, uint64_t C, const ConvGeom &g, uint64_t nnz_x, const uint32_t *x_rows,
                               const uint32_t *x_cols, const T *x_vals, uint64_t OC, uint64_t nnz_w, const uint32_t *w_rows,
                               const uint32_t *w_cols, const T *w_vals, osp_memspace_t space, const osp_config_t &cfg) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint32_t *xr = to_device(sc, x_rows, nnz_x, space, s), *xc = to_device(sc, x_cols, nnz_x, space, s);
    const uint32_t *wr = to_device(sc, w_rows, nnz_w, space, s), *wc = to_device(sc, w_cols, nnz_w, space, s);
    const T *xv = to_device(sc, x_vals, nnz_x, space, s), *wv = to_device(sc, w_vals, nnz_w, space, s);
    const uint64_t M = N * g.OH * g.OW, K = C * g.kh * g.kw;
    int64_t *ap = nullptr, *bp;
    uint32_t *ai = nullptr, *bi;
    T *av = nullptr, *bv;
    im2col_impl<T>(ctx, sc, N, C, g, nnz_x, xr, xc, xv, true, ap, ai, av);
    coo_to_compressed_device<T>(ctx, sc, K, OC, nnz_w, wc, wr, wv, "W (COO)", &bp, &bi, &bv);   // B = W^T in CSR = W in CSC
    OSP_HIP(hipEventRecord(ev.b, s));
    osp_config_t c2 = cfg;
    c2.validate = 0;  // A is well formed by construction; W's ranges and duplicates were just checked
    spgemm_impl<T>(ctx, res, M, K, OC, ap, ai, av, bp, bi, bv, OSP_DEVICE, c2);
    const float ms = ev.ms();
    res->info.ms_ingest = ms;
    res->info.ms_total += ms;
}

// MaxPool2d of a CSR activation, the zeros dropped, as a new CSR (osp_conv.h)
template <class T>
static void maxpool_impl(Context *ctx, const Result *in, Result *res, uint64_t N, uint32_t H, uint32_t W, uint32_t kh, uint32_t kw,
                         uint32_t sh, uint32_t sw) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint32_t C = (uint32_t)in->info.N, PH = (H - kh) / sh + 1, PW = (W - kw) / sw + 1;
    const uint64_t M = N * PH * PW;
    res->info = in->info;
    res->info.M = M;
    res->info.row_begin = 0;
    res->info.row_end = M;
    const unsigned grid = grid_for(std::max<uint64_t>(M, 1) * kWave, 256);
    const uint64_t nnz = rows_two_pass<T>(
        sc, res, M, s,
        [&](uint32_t *cnt) {
            csr_maxpool_rows_kernel<T, false><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, (const T *)in->vals, C, H, W, PH, PW, kh, kw, sh, sw, M, cnt,
                                                                   nullptr, nullptr, nullptr);
        },
        [&] {
            csr_maxpool_rows_kernel<T, true><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, (const T *)in->vals, C, H, W, PH, PW, kh, kw, sh, sw, M,
                                                                  nullptr, res->rowptr, res->colidx, (T *)res->vals);
        });
    finish_csr(res, ev, nnz, s);
}

// ---- the masked product (osp_masked.h) ----
// One operand in the other major order: (ptr, idx, vals) with nseg_minor segments -> (ptr_out over nseg_major segments,
// the old segment index in ascending order inside each, vals).  One stable sort by the new major index: entries of one new
// segment keep their input order, which is ascending in the old segment index.
template <class T>
static void masked_view(Context *ctx, Scratch &sc, uint64_t nseg_minor, uint64_t nseg_major, uint64_t nnz, const int64_t *ptr,
                        const uint32_t *idx, const T *vals, int64_t **ptr_out, uint32_t **idx_out, T **vals_out) {
    hipStream_t s = ctx->stream;
    int64_t *optr = sc.get<int64_t>(nseg_major + 1);
    uint32_t *oidx = sc.get<uint32_t>(nnz);
    T *ovals = sc.get<T>(nnz);
    *ptr_out = optr; *idx_out = oidx; *vals_out = ovals;
    if (nnz == 0) {
        OSP_HIP(hipMemsetAsync(optr, 0, (nseg_major + 1) * sizeof(int64_t), s));
        return;
    }
    Scratch ss(ctx);
    uint32_t *minor = ss.get<uint32_t>(nnz), *major = ss.get<uint32_t>(nnz);
    uint32_t *ka = ss.get<uint32_t>(nnz), *pa = ss.get<uint32_t>(nnz), *kb = ss.get<uint32_t>(nnz), *pb = ss.get<uint32_t>(nnz);
    uint32_t *hist = ss.get<uint32_t>(rs_hist_entries(nnz));
    uint32_t *hist_tmp = ss.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nnz)));
    if (nseg_minor) csr_expand_rows_kernel<<<grid_for(nseg_minor * kWave, 256), 256, 0, s>>>(ptr, nseg_minor, minor);
    device_sort_rows<MaskedViewEpilogue<T>>(idx, nnz, std::max(1, bits_for(nseg_major)), ka, pa, kb, pb, hist, hist_tmp,
                                            MaskedViewEpilogue<T>{minor, vals, major, oidx, ovals}, s, ctx->rank_atomic);
    ingest_ptr_kernel<<<grid_for(nseg_major + 1, 256), 256, 0, s>>>(major, nnz, nseg_major, optr);
    OSP_HIP(hipStreamSynchronize(s));   // (ss goes back to the pool)
}

// unsigned setting from the environment, or `dflt`
static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *v = getenv(name);
    return v && *v ? strtoull(v, nullptr, 10) : dflt;
}

template <class T>
static void masked_impl(Context *ctx, Result *res, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr_in, const uint32_t *a_rowidx_in,
                        const T *a_vals_in, const int64_t *b_rowptr_in, const uint32_t *b_colidx_in, const T *b_vals_in,
                        const int64_t *m_rowptr_in, const uint32_t *m_colidx_in, osp_memspace_t space, const osp_config_t &cfg) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev, ev_in, ev_k;
    OSP_HIP(hipEventRecord(ev.a, s));
    res->info = osp_result_info_t{};   // every field the masked product does not name stays 0 (rank_atomic included)
    res->info.dtype = res->dtype;
    res->info.M = M; res->info.K = K; res->info.N = N;
    res->info.row_begin = 0; res->info.row_end = M;

    const int64_t *a_colptr = to_device(sc, a_colptr_in, K + 1, space, s);
    const int64_t *b_rowptr = to_device(sc, b_rowptr_in, K + 1, space, s);
    const int64_t *m_rowptr = to_device(sc, m_rowptr_in, M + 1, space, s);
    int64_t nnz_a, nnz_b, nnz_m;
    if (space == OSP_HOST) {
        nnz_a = a_colptr_in[K]; nnz_b = b_rowptr_in[K]; nnz_m = m_rowptr_in[M];
    } else {
        Gather g(s);
        g.add(&nnz_a, a_colptr + K); g.add(&nnz_b, b_rowptr + K); g.add(&nnz_m, m_rowptr + M);
        g.wait();
    }
    if (nnz_a < 0 || nnz_b < 0 || nnz_m < 0) throw Error(OSP_ERR_ARG, "negative nnz in pointer array");
    if ((uint64_t)nnz_a >= 0xffffffffull || (uint64_t)nnz_b >= 0xffffffffull || (uint64_t)nnz_m >= 0xffffffffull)
        throw Error(OSP_ERR_ARG, "operands or masks with >= 2^32 non-zeros are not supported");
    if (nnz_m && !m_colidx_in) throw Error(OSP_ERR_ARG, "null mask column array with a non-empty mask");
    const uint32_t *a_rowidx = to_device(sc, a_rowidx_in, nnz_a, space, s);
    const T *a_vals = to_device(sc, a_vals_in, nnz_a, space, s);
    const uint32_t *b_colidx = to_device(sc, b_colidx_in, nnz_b, space, s);
    const T *b_vals = to_device(sc, b_vals_in, nnz_b, space, s);
    const uint32_t *m_colidx = to_device(sc, m_colidx_in, nnz_m, space, s);
    res->info.nnz_a = nnz_a;
    res->info.nnz_b = nnz_b;

    if (cfg.validate) {
        uint32_t *flags = sc.get<uint32_t>(3);
        OSP_HIP(hipMemsetAsync(flags, 0, 3 * sizeof(uint32_t), s));
        validate_ptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(a_colptr, K, nnz_a, flags);
        validate_ptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(b_rowptr, K, nnz_b, flags + 1);
        validate_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(m_rowptr, M, nnz_m, flags + 2);
        uint32_t f[3] = {0, 0, 0};
        { Gather g(s); for (int q = 0; q < 3; q++) g.add(&f[q], (const uint32_t *)flags + q); g.wait(); }
        check_flags(f[0], "A (CSC)");
        check_flags(f[1], "B (CSR)");
        check_flags(f[2], "mask (CSR)");
        if (nnz_a) validate_idx_kernel<<<grid_for(nnz_a, 256), 256, 0, s>>>(a_colptr, a_rowidx, K, nnz_a, M, flags);
        if (nnz_b) validate_idx_kernel<<<grid_for(nnz_b, 256), 256, 0, s>>>(b_rowptr, b_colidx, K, nnz_b, N, flags + 1);
        if (nnz_m) validate_idx_kernel<<<grid_for(nnz_m, 256), 256, 0, s>>>(m_rowptr, m_colidx, M, nnz_m, N, flags + 2);
        { Gather g(s); for (int q = 0; q < 3; q++) g.add(&f[q], (const uint32_t *)flags + q); g.wait(); }
        check_flags(f[0], "A (CSC)");
        check_flags(f[1], "B (CSR)");
        check_flags(f[2], "mask (CSR)");
    }

    // ---- views: A by rows, B by columns ----
    OSP_HIP(hipEventRecord(ev_in.a, s));
    int64_t *arow_ptr, *bcol_ptr;
    uint32_t *arow_k, *bcol_k;
    T *arow_v, *bcol_v;
    masked_view<T>(ctx, sc, K, M, nnz_a, a_colptr, a_rowidx, a_vals, &arow_ptr, &arow_k, &arow_v);
    masked_view<T>(ctx, sc, K, N, nnz_b, b_rowptr, b_colidx, b_vals, &bcol_ptr, &bcol_k, &bcol_v);
    OSP_HIP(hipEventRecord(ev_in.b, s));

    // ---- slots: classify, order light slots by cost bucket, intersect ----
    const uint64_t nm = (uint64_t)nnz_m;
    uint32_t *m_row = sc.get<uint32_t>(nm), *hit = sc.get<uint32_t>(nm);
    T *val = sc.get<T>(nm);
    unsigned long long *products = (unsigned long long *)sc.get<uint64_t>(1);
    uint32_t *count = sc.get<uint32_t>(kMaskedBuckets);
    zero_async(s, {{products, sizeof(uint64_t)}, {count, kMaskedBuckets * sizeof(uint32_t)}});
    uint32_t launches = 0;
    if (nm) {
        const uint32_t heavy_min = (uint32_t)std::min<uint64_t>(env_u64("OSP_MASKED_HEAVY_MIN", kMaskedHeavyMin), 0xffffffffull);
        const int bucketed = env_u64("OSP_MASKED_BUCKET", 1) ? 1 : 0;
        Scratch ss(ctx);
        uint32_t *key = ss.get<uint32_t>(nm), *order = ss.get<uint32_t>(nm);
        csr_expand_rows_kernel<<<grid_for(M * kWave, 256), 256, 0, s>>>(m_rowptr, M, m_row);
        masked_classify_kernel<<<grid_for(nm, 256), 256, 0, s>>>(m_row, m_colidx, arow_ptr, bcol_ptr, nm, heavy_min, bucketed, key, hit, count);
        uint32_t hc[kMaskedBuckets];
        copy_d2h(hc, count, sizeof(hc), s);
        const uint64_t n_empty = hc[kMaskedEmpty], n_heavy = hc[kMaskedHeavy], n_light = nm - n_empty - n_heavy;
        if (n_light || n_heavy) {
            uint32_t *ka = ss.get<uint32_t>(nm), *pa = ss.get<uint32_t>(nm), *kb = ss.get<uint32_t>(nm), *pb = ss.get<uint32_t>(nm);
            uint32_t *hist = ss.get<uint32_t>(rs_hist_entries(nm));
            uint32_t *hist_tmp = ss.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nm)));
            device_sort_rows<MaskedOrderEpilogue>(key, nm, 5, ka, pa, kb, pb, hist, hist_tmp, MaskedOrderEpilogue{order}, s, ctx->rank_atomic);
        }
        const MaskedOperands op{m_row, m_colidx, arow_ptr, arow_k, bcol_ptr, bcol_k};
        OSP_HIP(hipEventRecord(ev_k.a, s));
        if (n_light) {
            masked_light_kernel<T><<<grid_for(n_light, 256), 256, 0, s>>>(op, arow_v, bcol_v, order + n_empty, n_light, hit, val, products);
            launches++;
        }
        if (n_heavy) {
            masked_heavy_kernel<T><<<(unsigned)n_heavy, kWave, 0, s>>>(op, arow_v, bcol_v, order + n_empty + n_light, n_heavy, hit, val, products);
            launches++;
        }
        OSP_HIP(hipEventRecord(ev_k.b, s));
        OSP_HIP(hipStreamSynchronize(s));   // (ss goes back to the pool)
    } else {
        OSP_HIP(hipEventRecord(ev_k.a, s));
        OSP_HIP(hipEventRecord(ev_k.b, s));
    }

    // ---- compaction: C at its exact size ----
    uint64_t *pos = sc.get<uint64_t>(nm + 1);
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(nm + 1));
    device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{hit}, nm, pos, tmp, s);
    uint64_t nnz_c = 0, P = 0;
    { Gather g(s); g.add(&nnz_c, (const uint64_t *)pos + nm); g.add(&P, (const uint64_t *)products); g.wait(); }
    alloc_rowptr(res, M);
    alloc_entries<T>(res, nnz_c);
    masked_rowptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(m_rowptr, pos, M, res->rowptr);
    if (nnz_c) masked_scatter_kernel<T><<<grid_for(nm, 256), 256, 0, s>>>(hit, val, m_colidx, pos, nm, res->colidx, (T *)res->vals);
    finish_csr(res, ev, nnz_c, s);
    res->info.partials = P;
    res->info.ms_ingest = ev_in.ms();
    res->info.ms_multiply_kernel = ev_k.ms();
    res->info.multiply_launches = launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] masked M=%llu K=%llu N=%llu nnzA=%lld nnzB=%lld nnzM=%lld nnzC=%llu products=%llu launches=%u %.3f ms\n",
                (unsigned long long)M, (unsigned long long)K, (unsigned long long)N, (long long)nnz_a, (long long)nnz_b, (long long)nnz_m,
                (unsigned long long)nnz_c, (unsigned long long)P, launches, res->info.ms_total);
}

// ---- the step between two expansions of Markov clustering (osp_mcl.h) ----
template <class T>
static void inflate_prune_impl(Context *ctx, const Result *in, Result *res, const osp_mcl_step_t &step, int validate, osp_mcl_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev, ev_k;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, nnz_in = in->info.nnz_c;
    const T *val = (const T *)in->vals;
    const T thr = (T)step.threshold, power = (T)step.power;
    const int mode = step.power == 1.0 ? MCL_POW_ONE : step.power == 2.0 ? MCL_POW_SQUARE : MCL_POW_GENERAL;
    const uint32_t long_min = (uint32_t)std::min<uint64_t>(env_u64("OSP_MCL_LONG_MIN", kMclLongMin), 0xffffffffull);
    uint32_t launches = 0;

    unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(MCL_COUNTERS);
    zero_async(s, {{counters, MCL_COUNTERS * sizeof(uint64_t)}});
    if (validate && nnz_in) {
        mcl_validate_kernel<T><<<grid_for(nnz_in, 256), 256, 0, s>>>(val, nnz_in, counters);
        launches++;
        if (d2h((const uint64_t *)counters + MCL_INVALID, s)) throw Error(OSP_ERR_ARG, "inflate_prune: a value is negative, NaN or infinite");
    }

    // ---- classes: rows longer than long_min get a workgroup each ----
    uint32_t *long_rows = sc.get<uint32_t>(nnz_in / ((uint64_t)long_min + 1) + 1);
    if (M) {
        mcl_classify_kernel<<<grid_for(M, 256), 256, 0, s>>>(in->rowptr, M, long_min, long_rows, counters);
        launches++;
    }
    const uint64_t n_long = d2h((const uint64_t *)counters + MCL_NLONG, s);

    // ---- pass 1: kept entries per row, then the output's row pointers ----
    res->info = in->info;
    uint32_t *nsurv = sc.get<uint32_t>(M + 1);
    constexpr uint64_t kSlice = 1ull << 30;   // rows per launch of the one-wave-per-row kernels (grid limit)
    const uint64_t nnz = rows_two_pass<T>(
        sc, res, M, s,
        [&](uint32_t *cnt) {
            for (uint64_t r0 = 0; r0 < M; r0 += kSlice) {
                mcl_count_kernel<T, kWave><<<(unsigned)std::min(kSlice, M - r0), kWave, 0, s>>>(in->rowptr, val, r0, M, nullptr, long_min, thr,
                                                                                              step.max_per_row, nsurv, cnt, counters);
                launches++;
            }
            if (n_long) {
                mcl_count_kernel<T, kMclLongThreads><<<(unsigned)n_long, kMclLongThreads, 0, s>>>(in->rowptr, val, 0, M, long_rows, long_min, thr,
                                                                                                  step.max_per_row, nsurv, cnt, counters);
                launches++;
            }
        },
        // ---- pass 2: select, compact, inflate, normalise ----
        [&] {
            OSP_HIP(hipEventRecord(ev_k.a, s));
            for (uint64_t r0 = 0; r0 < M; r0 += kSlice) {
                mcl_write_kernel<T, kWave><<<(unsigned)std::min(kSlice, M - r0), kWave, 0, s>>>(in->rowptr, in->colidx, val, r0, M, nullptr, long_min, thr,
                                                                                              mode, power, nsurv, res->rowptr, res->colidx,
                                                                                              (T *)res->vals, counters);
                launches++;
            }
            if (n_long) {
                mcl_write_kernel<T, kMclLongThreads><<<(unsigned)n_long, kMclLongThreads, 0, s>>>(in->rowptr, in->colidx, val, 0, M, long_rows, long_min,
                                                                                                  thr, mode, power, nsurv, res->rowptr, res->colidx,
                                                                                                  (T *)res->vals, counters);
                launches++;
            }
            OSP_HIP(hipEventRecord(ev_k.b, s));
        });
    if (!nnz) {   // (no second pass: an empty interval)
        OSP_HIP(hipEventRecord(ev_k.a, s));
        OSP_HIP(hipEventRecord(ev_k.b, s));
    }
    uint64_t capped = 0, rescued = 0, chaos_bits = 0;
    {
        Gather g(s);
        g.add(&capped, (const uint64_t *)counters + MCL_CAPPED);
        g.add(&rescued, (const uint64_t *)counters + MCL_RESCUED);
        g.add(&chaos_bits, (const uint64_t *)counters + MCL_CHAOS);
        g.wait();
    }
    finish_csr(res, ev, nnz, s);
    *st = osp_mcl_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = nnz;
    st->rows_capped = capped;
    st->rows_rescued = rescued;
    st->rows_long = n_long;
    if (sizeof(T) == 8) {
        memcpy(&st->chaos, &chaos_bits, 8);
    } else {
        const uint32_t b32 = (uint32_t)chaos_bits;
        float f;
        memcpy(&f, &b32, 4);
        st->chaos = (double)f;
    }
    st->ms_total = res->info.ms_total;
    st->ms_select_kernel = ev_k.ms();
    st->launches = launches + 1;   // (the counters' zeroing)
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] inflate_prune M=%llu nnz %llu -> %llu capped=%llu rescued=%llu long=%llu chaos=%.3e %.3f ms (select %.3f)\n",
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)nnz, (unsigned long long)capped, (unsigned long long)rescued,
                (unsigned long long)n_long, st->chaos, st->ms_total, st->ms_select_kernel);
}

// ---- the mask filter C<M> / C<¬M> of a CSR result (osp_apply_mask.h) ----
template <class T>
static void apply_mask_impl(Context *ctx, const Result *in, Result *res, const int64_t *m_rowptr_in, const uint32_t *m_colidx_in,
                            osp_memspace_t space, int complement, int validate, osp_apply_mask_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz_in = in->info.nnz_c;
    uint32_t launches = 0;

    // ---- the mask; a device mask's nnz comes back with nnz_out unless something needs it earlier ----
    const int64_t *m_rowptr = to_device(sc, m_rowptr_in, M + 1, space, s);
    int64_t nnz_m = 0;
    bool have_nnz_m = space == OSP_HOST;
    if (have_nnz_m) nnz_m = m_rowptr_in[M];
    const auto check_nnz_m = [&] {
        if (nnz_m < 0) throw Error(OSP_ERR_ARG, "apply_mask: negative nnz in the mask's pointer array");
        if ((uint64_t)nnz_m >= 0xffffffffull) throw Error(OSP_ERR_ARG, "apply_mask: masks with >= 2^32 non-zeros are not supported");
        if (nnz_m && !m_colidx_in) throw Error(OSP_ERR_ARG, "apply_mask: null mask column array with a non-empty mask");
    };
    if (!have_nnz_m && (!m_colidx_in || validate || nnz_in == 0)) {
        nnz_m = d2h(m_rowptr + M, s);
        have_nnz_m = true;
    }
    if (have_nnz_m) check_nnz_m();
    const uint32_t *m_colidx = space == OSP_HOST ? to_device(sc, m_colidx_in, (uint64_t)nnz_m, space, s) : m_colidx_in;

    if (validate) {
        uint32_t *flags = sc.get<uint32_t>(1);
        zero_async(s, {{flags, sizeof(uint32_t)}});
        validate_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(m_rowptr, M, (uint64_t)nnz_m, flags);
        launches += 2;
        check_flags(d2h((const uint32_t *)flags, s), "mask (CSR)");
        if (nnz_m) {
            validate_idx_kernel<<<grid_for((uint64_t)nnz_m, 256), 256, 0, s>>>(m_rowptr, m_colidx, M, (uint64_t)nnz_m, N, flags);
            launches++;
            check_flags(d2h((const uint32_t *)flags, s), "mask (CSR)");
        }
    }

    res->info = in->info;
    Compacted c{0, 0};
    if (nnz_in && complement && have_nnz_m && nnz_m == 0) {
        // nothing is masked out: `in` itself
        c.nnz = nnz_in;
        alloc_rowptr(res, M);
        OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        alloc_entries<T>(res, nnz_in);
        OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz_in * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        OSP_HIP(hipMemcpyAsync(res->vals, in->vals, nnz_in * sizeof(T), hipMemcpyDeviceToDevice, s));
    } else if (have_nnz_m && nnz_m == 0) {
        empty_result<T>(res, M, s);   // nothing to search for
    } else {
        c = compact_by_bits<T>(
            sc, in, res, s,
            [&](unsigned nchunks, uint64_t *bits) {
                apply_mask_flag_kernel<<<nchunks, kAmThreads, 0, s>>>(in->rowptr, in->colidx, M, nnz_in, m_rowptr, m_colidx, complement, bits);
            },
            nullptr, [&](Gather &g) { if (!have_nnz_m) g.add(&nnz_m, m_rowptr + M); });
        if (!have_nnz_m) check_nnz_m();
        launches += c.launches;
    }
    finish_csr(res, ev, c.nnz, s);
    *st = osp_apply_mask_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_mask = (uint64_t)nnz_m;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] apply_mask%s M=%llu nnz %llu -> %llu (mask %llu) launches=%u %.3f ms\n", complement ? " (complement)" : "",
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)c.nnz, (unsigned long long)nnz_m, launches, st->ms_total);
}

// ---- the entry filter of a CSR result (osp_select.h) ----
template <class T, int OP = 0>
static void launch_select_value(int op, unsigned grid, hipStream_t s, const T *val, uint64_t nnz, double threshold, uint64_t *bits) {
    if constexpr (OP <= SEL_NE) {
        if (op == OP) select_flag_value_kernel<T, OP><<<grid, kCompactThreads, 0, s>>>(val, nnz, threshold, bits);
        else launch_select_value<T, OP + 1>(op, grid, s, val, nnz, threshold, bits);
    }
}
template <int OP = SEL_TRIL>
static void launch_select_position(int op, unsigned grid, hipStream_t s, const int64_t *rowptr, const uint32_t *col, uint64_t M, uint64_t nnz,
                                   int64_t diag, uint64_t *bits) {
    if constexpr (OP < SEL_OPS) {
        if (op == OP) select_flag_position_kernel<OP><<<grid, kCompactThreads, 0, s>>>(rowptr, col, M, nnz, diag, bits);
        else launch_select_position<OP + 1>(op, grid, s, rowptr, col, M, nnz, diag, bits);
    }
}

template <class T>
static void select_impl(Context *ctx, const Result *in, Result *res, const osp_select_t &sel, osp_select_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, nnz_in = in->info.nnz_c;
    res->info = in->info;
    // (a double beyond T's range has no defined conversion: it becomes the infinity of its sign)
    const double fv = sel.fill_value;
    const T fill = std::isfinite(fv) && std::fabs(fv) > (double)std::numeric_limits<T>::max()
                       ? (T)std::copysign((double)std::numeric_limits<T>::infinity(), fv) : (T)fv;
    const Compacted c = compact_by_bits<T>(
        sc, in, res, s,
        [&](unsigned nchunks, uint64_t *bits) {
            if (sel.op <= OSP_SELECT_NE) {
                launch_select_value<T>(sel.op, nchunks, s, (const T *)in->vals, nnz_in, sel.threshold, bits);
            } else {
                // |col - row| < 2^32: a diagonal beyond +-2^33 selects what +-2^33 selects, and row + diag cannot overflow
                const int64_t lim = (int64_t)1 << 33;
                launch_select_position(sel.op, nchunks, s, in->rowptr, in->colidx, M, nnz_in, std::min(std::max(sel.diag, -lim), lim), bits);
            }
        },
        sel.fill ? &fill : nullptr);
    finish_csr(res, ev, c.nnz, s);
    *st = osp_select_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = c.launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] select op=%d%s M=%llu nnz %llu -> %llu launches=%u %.3f ms\n", sel.op, sel.fill ? " (fill)" : "",
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)c.nnz, c.launches, st->ms_total);
}

// ---- the element-wise union / intersection of two CSR results (osp_ewise.h) ----
template <class T, int OP = 0>
static void launch_ewise_union_a(int op, unsigned grid, hipStream_t s, const Result *a, const Result *b, const BitScan &h, Result *res) {
    typedef ValueBits<T> V;
    if constexpr (OP <= EW_SECOND) {
        if (op == OP)
            ewise_union_write_a_kernel<T, OP><<<grid, kCompactThreads, 0, s>>>(a->rowptr, a->colidx, (const V *)a->vals, a->info.M, a->info.nnz_c,
                                                                              b->rowptr, b->colidx, (const V *)b->vals, h.bits, h.pos, res->colidx,
                                                                              (V *)res->vals);
        else launch_ewise_union_a<T, OP + 1>(op, grid, s, a, b, h, res);
    }
}
template <class T, int OP = 0>
static void launch_ewise_intersect(int op, unsigned grid, hipStream_t s, const Result *a, const Result *b, const BitScan &h, const uint32_t *qpos,
                                   Result *res) {
    typedef ValueBits<T> V;
    if constexpr (OP < EW_OPS) {
        if (op == OP)
            ewise_intersect_write_kernel<T, OP><<<grid, 256, 0, s>>>(a->colidx, (const V *)a->vals, a->info.nnz_c, (const V *)b->vals, h.bits, h.pos,
                                                                     qpos, res->colidx, (V *)res->vals);
        else launch_ewise_intersect<T, OP + 1>(op, grid, s, a, b, h, qpos, res);
    }
}

template <class T>
static void copy_csr(const Result *in, Result *res, hipStream_t s) {
    const uint64_t M = in->info.M, nnz = in->info.nnz_c;
    alloc_rowptr(res, M);
    OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    alloc_entries<T>(res, nnz);
    OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    OSP_HIP(hipMemcpyAsync(res->vals, in->vals, nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
}

template <class T>
static void ewise_impl(Context *ctx, const Result *a, const Result *b, Result *res, const osp_ewise_t &ew, osp_ewise_stats_t *st) {
    typedef ValueBits<T> V;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = a->info.M, nnz_a = a->info.nnz_c, nnz_b = b->info.nnz_c;
    const bool uni = ew.mode == OSP_EWISE_UNION;
    res->info = a->info;
    uint64_t nnz_both = 0, nnz_out = 0;
    uint32_t launches = 0;
    if (M == 0 || (uni ? nnz_a + nnz_b == 0 : nnz_a == 0 || nnz_b == 0)) {
        empty_result<T>(res, M, s);
    } else if (nnz_a == 0 || nnz_b == 0) {
        // a union with an empty side: the other side
        copy_csr<T>(nnz_a ? a : b, res, s);
        nnz_out = nnz_a + nnz_b;
    } else if (uni) {
        // the flag runs over b: hitsB, and every entry of b's lower bound in a
        uint32_t *qpos = sc.get<uint32_t>(nnz_b);
        alloc_rowptr(res, M);
        const BitScan h = flag_and_scan(sc, nnz_b, s, [&](unsigned nchunks, uint64_t *bits) {
            ewise_flag_kernel<<<nchunks, kCompactThreads, 0, s>>>(b->rowptr, b->colidx, M, nnz_b, a->rowptr, a->colidx, bits, qpos);
        });
        nnz_both = h.count;
        nnz_out = nnz_a + nnz_b - nnz_both;
        alloc_entries<T>(res, nnz_out);
        ewise_union_rowptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(a->rowptr, b->rowptr, M, h.bits, h.pos, res->rowptr);
        launches = h.launches + 2;
        if (nnz_both < nnz_b) {   // (else b has no entry of its own)
            ewise_union_write_b_kernel<V><<<grid_for(nnz_b, 256), 256, 0, s>>>(b->colidx, (const V *)b->vals, nnz_b, h.bits, h.pos, qpos, res->colidx,
                                                                               (V *)res->vals);
            launches++;
        }
        launch_ewise_union_a<T>(ew.op, grid_for(nnz_a, (unsigned)kCompactChunk), s, a, b, h, res);
    } else {
        // the flag runs over a: the common entries are a's with their bit set, b's value is at the stored lower bound
        uint32_t *qpos = sc.get<uint32_t>(nnz_a);
        alloc_rowptr(res, M);
        const BitScan h = flag_and_scan(sc, nnz_a, s, [&](unsigned nchunks, uint64_t *bits) {
            ewise_flag_kernel<<<nchunks, kCompactThreads, 0, s>>>(a->rowptr, a->colidx, M, nnz_a, b->rowptr, b->colidx, bits, qpos);
        });
        nnz_both = nnz_out = h.count;
        alloc_entries<T>(res, nnz_out);
        compact_rowptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(a->rowptr, M, h.bits, h.pos, res->rowptr);
        launches = h.launches + 1;
        if (nnz_out) {
            launch_ewise_intersect<T>(ew.op, grid_for(nnz_a, 256), s, a, b, h, qpos, res);
            launches++;
        }
    }
    finish_csr(res, ev, nnz_out, s);
    *st = osp_ewise_stats_t{};
    st->nnz_a = nnz_a;
    st->nnz_b = nnz_b;
    st->nnz_both = nnz_both;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] ewise %s op=%d M=%llu nnz %llu , %llu -> %llu (both %llu) launches=%u %.3f ms\n", uni ? "union" : "intersect", ew.op,
                (unsigned long long)M, (unsigned long long)nnz_a, (unsigned long long)nnz_b, (unsigned long long)nnz_out,
                (unsigned long long)nnz_both, launches, st->ms_total);
}

// ---- the product of two CSR results under a semiring (osp_mxm.h) ----
struct MxmOperands {
    const int64_t *a_rowptr; const uint32_t *a_col; const void *a_val;
    const int64_t *b_rowptr; const uint32_t *b_col; const void *b_val;
    const uint64_t *wscan;
};
template <class T, int ADD>
static void launch_mxm_short_add(const MxmOperands &op, hipStream_t s, uint64_t r0, uint64_t nrows, uint32_t cap, int mul, uint64_t p0, uint32_t *tcol,
                                 ValueBits<T> *tval, uint32_t *cnt) {
    typedef ValueBits<T> V;
    mxm_short_kernel<T, ADD><<<(unsigned)nrows, kWave, 0, s>>>(op.a_rowptr, op.a_col, (const V *)op.a_val, op.b_rowptr, op.b_col, (const V *)op.b_val,
                                                                op.wscan, r0, cap, mul, p0, tcol, tval, cnt);
}
template <class T>
static void launch_mxm_short(int add, const MxmOperands &op, hipStream_t s, uint64_t r0, uint64_t nrows, uint32_t cap, int mul, uint64_t p0,
                             uint32_t *tcol, ValueBits<T> *tval, uint32_t *cnt) {
    if (add == EW_PLUS) launch_mxm_short_add<T, EW_PLUS>(op, s, r0, nrows, cap, mul, p0, tcol, tval, cnt);
    else if (add == EW_MIN) launch_mxm_short_add<T, EW_MIN>(op, s, r0, nrows, cap, mul, p0, tcol, tval, cnt);
    else if (add == EW_MAX) launch_mxm_short_add<T, EW_MAX>(op, s, r0, nrows, cap, mul, p0, tcol, tval, cnt);
    else launch_mxm_short_add<T, EW_FIRST>(op, s, r0, nrows, cap, mul, p0, tcol, tval, cnt);
}
template <class T, int MUL = 0>
static void launch_mxm_expand(int mul, const MxmOperands &op, hipStream_t s, const uint32_t *long_rows, const uint64_t *loff, uint32_t nlong,
                              uint64_t nprod, int colbits, uint64_t *key, uint32_t *pos, ValueBits<T> *pval) {
    typedef ValueBits<T> V;
    if constexpr (MUL <= EW_SECOND) {
        if (mul == MUL)
            mxm_expand_kernel<T, MUL><<<grid_for(nprod, 256), 256, 0, s>>>(op.a_rowptr, op.a_col, (const V *)op.a_val, op.b_rowptr, op.b_col,
                                                                          (const V *)op.b_val, op.wscan, long_rows, loff, nlong, nprod, colbits, key,
                                                                          pos, pval);
        else launch_mxm_expand<T, MUL + 1>(mul, op, s, long_rows, loff, nlong, nprod, colbits, key, pos, pval);
    }
}
template <class T, int ADD>
static void launch_mxm_fold_add(const MxmOperands &op, hipStream_t s, const uint64_t *key, const ValueBits<T> *sorted_val, const uint64_t *headscan,
                                const uint64_t *head_pos, uint64_t nprod, const uint32_t *long_rows, const uint64_t *loff, int colbits, uint64_t p0,
                                uint32_t *tcol, ValueBits<T> *tval) {
    mxm_fold_kernel<T, ADD><<<grid_for(nprod, 256), 256, 0, s>>>(key, sorted_val, headscan, head_pos, nprod, op.a_rowptr, op.wscan, long_rows, loff,
                                                                 colbits, p0, tcol, tval);
}
// kernels of one device_exclusive_scan over n entries
static uint32_t scan_launches(uint64_t n) { return n == 0 || (n + kScanTile - 1) / kScanTile <= kScanSmallTiles ? 1u : 3u; }

template <class T>
static void mxm_impl(Context *ctx, const Result *a, const Result *b, Result *res, const osp_semiring_t &sr, osp_mxm_stats_t *st) {
    typedef ValueBits<T> V;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = a->info.M, K = a->info.N, N = b->info.N, nnz_a = a->info.nnz_c, nnz_b = b->info.nnz_c;
    res->info = osp_result_info_t{};   // every field the product does not name stays 0
    res->info.dtype = res->dtype;
    res->info.M = M; res->info.K = K; res->info.N = N;
    res->info.row_begin = 0; res->info.row_end = M;
    res->info.nnz_a = nnz_a; res->info.nnz_b = nnz_b;
    uint64_t products = 0, nnz_out = 0, n_short = 0, n_long = 0;
    uint32_t nb = 0, launches = 0;

    // ---- symbolic: the products of every entry of a, scanned ----
    uint64_t *wscan = nullptr;
    if (M && nnz_a && nnz_b) {
        uint32_t *w = sc.get<uint32_t>(nnz_a);
        wscan = sc.get<uint64_t>(nnz_a + 1);
        uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(nnz_a));
        mxm_entry_len_kernel<<<grid_for(nnz_a, 256), 256, 0, s>>>(a->colidx, nnz_a, b->rowptr, w);
        launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{w}, nnz_a, wscan, tmp, s);
        products = d2h((const uint64_t *)wscan + nnz_a, s);
    }
    if (products == 0) {
        empty_result<T>(res, M, s);
    } else {
        const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(env_u64("OSP_MXM_SHORT_CAP", kMxmShortMax), 1), kMxmShortMax);
        const uint64_t budget = std::min<uint64_t>(std::max<uint64_t>(env_u64("OSP_MXM_BATCH", kMxmBatchDefault), 1), 0xfffffffeull);
        const MxmOperands op{a->rowptr, a->colidx, a->vals, b->rowptr, b->colidx, b->vals, wscan};
        // ---- the rows' classes and the batches ----
        // (two consecutive batches hold more than `budget` products between them, or the cut would not lie there)
        const uint32_t max_batches = (uint32_t)std::min<uint64_t>(M, 2 * (products / budget) + 3);
        unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(MXM_COUNTERS);
        uint64_t *cuts = sc.get<uint64_t>(2 * ((uint64_t)max_batches + 1));
        uint32_t *d_nb = sc.get<uint32_t>(1);
        zero_async(s, {{counters, MXM_COUNTERS * sizeof(uint64_t)}});
        mxm_classify_kernel<<<grid_for(M, 256), 256, 0, s>>>(a->rowptr, M, wscan, cap, counters);
        mxm_cut_kernel<<<1, 1, 0, s>>>(a->rowptr, wscan, M, budget, max_batches, cuts, d_nb);
        launches += 3;
        uint64_t n_toobig = 0;
        {
            Gather g(s);
            g.add(&n_short, (const uint64_t *)counters + MXM_NSHORT);
            g.add(&n_long, (const uint64_t *)counters + MXM_NLONG);
            g.add(&n_toobig, (const uint64_t *)counters + MXM_NTOOBIG);
            g.add(&nb, (const uint32_t *)d_nb);
            g.wait();
        }
        if (n_toobig) throw Error(OSP_ERR_CAPACITY, "mxm: an output row has >= 2^32 - 1 products (positions inside a batch are 32 bits)");
        if (nb > max_batches) throw Error(OSP_ERR_CAPACITY, "mxm: the batch list overflowed its bound");
        std::vector<uint64_t> cut((size_t)2 * (nb + 1));
        copy_d2h(cut.data(), cuts, cut.size() * sizeof(uint64_t), s);

        alloc_rowptr(res, M);
        uint32_t *cnt = sc.get<uint32_t>(M + 1);
        const int colbits = bits_for(N);
        struct BatchOut { uint32_t *col; V *val; uint64_t nnz; };
        std::vector<BatchOut> outs;
        for (uint32_t t = 0; t < nb; t++) {
            const uint64_t r0 = cut[2 * t], p0 = cut[2 * t + 1], nrows = cut[2 * t + 2] - r0, pb = cut[2 * t + 3] - p0;
            Scratch sb(ctx);
            // a row's slot is its place in the batch's expansion: it holds at most as many entries as the row has products
            uint32_t *tcol = sb.get<uint32_t>(pb);
            V *tval = sb.get<V>(pb);
            launch_mxm_short<T>(sr.add, op, s, r0, nrows, cap, sr.mul, p0, tcol, tval, cnt);
            launches++;
            if (n_long) {
                uint32_t *flag = sb.get<uint32_t>(nrows + 1), *lp = sb.get<uint32_t>(nrows + 1);
                uint64_t *rank = sb.get<uint64_t>(nrows + 1), *lpscan = sb.get<uint64_t>(nrows + 1);
                uint64_t *tmp = sb.get<uint64_t>(scan_scratch_entries(nrows + 1));
                mxm_long_flag_kernel<<<grid_for(nrows, 256), 256, 0, s>>>(a->rowptr, wscan, r0, nrows, cap, flag, lp);
                launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{flag}, nrows, rank, tmp, s);
                launches += device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{lp}, nrows, lpscan, tmp, s);
                uint64_t nl = 0, pl = 0;
                { Gather g(s); g.add(&nl, (const uint64_t *)rank + nrows); g.add(&pl, (const uint64_t *)lpscan + nrows); g.wait(); }
                if (nl) {
                    uint32_t *long_rows = sb.get<uint32_t>(nl);
                    uint64_t *loff = sb.get<uint64_t>(nl + 1);
                    mxm_long_list_kernel<<<grid_for(nrows + 1, 256), 256, 0, s>>>(flag, rank, lpscan, r0, nrows, long_rows, loff);
                    uint64_t *keys[2] = {sb.get<uint64_t>(pl + 1), sb.get<uint64_t>(pl + 1)};   // +1: the idle one holds the run heads later
                    uint32_t *poss[2] = {sb.get<uint32_t>(pl), sb.get<uint32_t>(pl)};
                    uint32_t *hist = sb.get<uint32_t>(sort_hist_entries(pl));
                    uint32_t *hist_tmp = sb.get<uint32_t>(scan_scratch_entries(sort_hist_entries(pl)));
                    V *pval = sb.get<V>(pl), *sorted_val = sb.get<V>(pl);
                    launch_mxm_expand<T>(sr.mul, op, s, long_rows, loff, (uint32_t)nl, pl, colbits, keys[0], poss[0], pval);
                    const int nbits = colbits + bits_for(nl);
                    const int cur = device_radix_sort_pairs<uint64_t>(keys, poss, pl, nbits, hist, hist_tmp, s, ctx->rank_atomic);
                    launches += 2 + (uint32_t)((nbits + 7) / 8) * (2 + scan_launches(sort_blocks(pl) * kRadix));
                    mxm_sorted_values_kernel<V><<<grid_for(pl, 256), 256, 0, s>>>(poss[cur], pval, pl, sorted_val);
                    uint64_t *headscan = sb.get<uint64_t>(pl + 1);
                    uint64_t *headscan_tmp = sb.get<uint64_t>(scan_scratch_entries(pl));
                    launches += 1 + device_exclusive_scan<HeavyHeadFlag, uint64_t>(HeavyHeadFlag{keys[cur]}, pl, headscan, headscan_tmp, s);
                    uint64_t *head_pos = keys[cur ^ 1];   // one entry per run and a sentinel, <= pl + 1
                    heavy_heads_kernel<<<grid_for(pl + 1, 256), 256, 0, s>>>(keys[cur], headscan, pl, head_pos);
                    if (sr.add == EW_PLUS) launch_mxm_fold_add<T, EW_PLUS>(op, s, keys[cur], sorted_val, headscan, head_pos, pl, long_rows, loff, colbits, p0, tcol, tval);
                    else if (sr.add == EW_MIN) launch_mxm_fold_add<T, EW_MIN>(op, s, keys[cur], sorted_val, headscan, head_pos, pl, long_rows, loff, colbits, p0, tcol, tval);
                    else if (sr.add == EW_MAX) launch_mxm_fold_add<T, EW_MAX>(op, s, keys[cur], sorted_val, headscan, head_pos, pl, long_rows, loff, colbits, p0, tcol, tval);
                    else launch_mxm_fold_add<T, EW_FIRST>(op, s, keys[cur], sorted_val, headscan, head_pos, pl, long_rows, loff, colbits, p0, tcol, tval);
                    mxm_long_counts_kernel<<<grid_for(nl, 256), 256, 0, s>>>(long_rows, loff, (uint32_t)nl, headscan, cnt);
                    launches += 3;
                }
            }
            // the batch's output at its exact size: the scan of its rows' counts, ONE read-back, the slots' entries gathered
            uint64_t *bptr = nb == 1 ? (uint64_t *)res->rowptr : sb.get<uint64_t>(nrows + 1);
            uint64_t *tmp = sb.get<uint64_t>(scan_scratch_entries(nrows + 1));
            launches += device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{cnt + r0}, nrows, bptr, tmp, s);
            const uint64_t nnz_b_out = d2h((const uint64_t *)bptr + nrows, s);
            BatchOut o{nullptr, nullptr, nnz_b_out};
            if (nb == 1) {
                alloc_entries<T>(res, nnz_b_out);
                o.col = res->colidx;
                o.val = (V *)res->vals;
            } else {
                o.col = sc.get<uint32_t>(nnz_b_out);
                o.val = sc.get<V>(nnz_b_out);
            }
            if (nnz_b_out) {
                mxm_gather_kernel<V><<<grid_for(nnz_b_out, 256), 256, 0, s>>>(a->rowptr, wscan, r0, nrows, p0, bptr, nnz_b_out, tcol, tval, o.col, o.val);
                launches++;
            }
            outs.push_back(o);
            nnz_out += nnz_b_out;
            OSP_HIP(hipStreamSynchronize(s));   // (sb goes back to the pool)
        }
        if (nb > 1) {
            // the result is the batches' outputs one after another, its row pointer the scan of all rows' counts
            uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(M + 1));
            launches += device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{cnt}, M, (uint64_t *)res->rowptr, tmp, s);
            alloc_entries<T>(res, nnz_out);
            uint64_t at = 0;
            for (const BatchOut &o : outs) {
                if (!o.nnz) continue;
                OSP_HIP(hipMemcpyAsync(res->colidx + at, o.col, o.nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
                OSP_HIP(hipMemcpyAsync((V *)res->vals + at, o.val, o.nnz * sizeof(V), hipMemcpyDeviceToDevice, s));
                at += o.nnz;
            }
        }
    }
    finish_csr(res, ev, nnz_out, s);
    res->info.partials = products;
    *st = osp_mxm_stats_t{};
    st->nnz_a = nnz_a;
    st->nnz_b = nnz_b;
    st->products = products;
    st->nnz_out = nnz_out;
    st->short_rows = n_short;
    st->long_rows = n_long;
    st->batches = nb;
    st->launches = launches;
    st->ms_total = res->info.ms_total;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] mxm add=%d mul=%d M=%llu K=%llu N=%llu nnz %llu , %llu -> %llu products=%llu short=%llu long=%llu batches=%u launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)K, (unsigned long long)N, (unsigned long long)nnz_a,
                (unsigned long long)nnz_b, (unsigned long long)nnz_out, (unsigned long long)products, (unsigned long long)n_short,
                (unsigned long long)n_long, nb, launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- the transpose of a CSR result (osp_transpose.h) ----
static bool env_is(const char *name, const char *value) {
    const char *e = getenv(name);
    return e && strcmp(e, value) == 0;
}

template <class T>
static void transpose_impl(Context *ctx, const Result *in, Result *res, osp_transpose_stats_t *st) {
    typedef ValueBits<T> V;
    typedef typename TrRecord<V>::type Rec;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    res->info = osp_result_info_t{};   // every field the transpose does not name stays 0
    res->info.dtype = res->dtype;
    res->info.M = N; res->info.K = in->info.K; res->info.N = M;
    res->info.row_begin = 0; res->info.row_end = N;
    res->info.nnz_a = nnz;
    uint32_t path = 0, passes = 0, launches = 0;
    if (nnz == 0) {
        empty_result<T>(res, N, s);
    } else if (M <= kTrMaskRows && !env_is("OSP_TRANSPOSE_PATH", "sort")) {
        path = 1;
        alloc_rowptr(res, N);
        alloc_entries<T>(res, nnz);
        // (pool buffers are recycled, and OSP_POISON fills them: the words are zeroed on every call)
        uint64_t *mask = sc.get<uint64_t>(N);
        uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(N));
        OSP_HIP(hipMemsetAsync(mask, 0, N * sizeof(uint64_t), s));
        const unsigned nchunks = grid_for(nnz, (unsigned)kCompactChunk);
        tr_rowmask_kernel<<<nchunks, kCompactThreads, 0, s>>>(in->rowptr, in->colidx, M, N, nnz, (unsigned long long *)mask);
        launches = 1 + device_exclusive_scan<LoadPopc64, uint64_t>(LoadPopc64{mask}, N, (uint64_t *)res->rowptr, tmp, s);
        tr_place_kernel<V><<<nchunks, kCompactThreads, 0, s>>>(in->rowptr, in->colidx, (const V *)in->vals, M, N, nnz, mask, res->rowptr,
                                                              res->colidx, (V *)res->vals);
        launches++;
    } else {
        path = 2;
        alloc_rowptr(res, N);
        alloc_entries<T>(res, nnz);
        const int nbits = std::max(1, bits_for(N));   // the bits of N - 1
        passes = (uint32_t)((nbits + 7) / 8);
        // the sort's (key, position) pairs between two passes: none with one pass, one pair of arrays with two
        uint32_t *ka = nullptr, *pa = nullptr, *kb = nullptr, *pb = nullptr;
        if (passes > 1) { ka = sc.get<uint32_t>(nnz); pa = sc.get<uint32_t>(nnz); }
        if (passes > 2) { kb = sc.get<uint32_t>(nnz); pb = sc.get<uint32_t>(nnz); }
        uint32_t *hist = sc.get<uint32_t>(rs_hist_entries(nnz));
        uint32_t *hist_tmp = sc.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nnz)));
        uint32_t *sorted_cols = sc.get<uint32_t>(nnz);
        if (env_is("OSP_TRANSPOSE_GATHER", "bisect")) {
            const TrEpilogue<V, false> epi{nullptr, in->rowptr, (const V *)in->vals, M, res->colidx, sorted_cols, (V *)res->vals};
            device_sort_rows(in->colidx, nnz, nbits, ka, pa, kb, pb, hist, hist_tmp, epi, s, ctx->rank_atomic);
        } else {
            Rec *rec = sc.get<Rec>(nnz);
            tr_pack_kernel<V><<<grid_for(nnz, (unsigned)kCompactChunk), kCompactThreads, 0, s>>>(in->rowptr, in->colidx, (const V *)in->vals, M, nnz, rec);
            launches++;
            const TrEpilogue<V, true> epi{rec, nullptr, nullptr, M, res->colidx, sorted_cols, (V *)res->vals};
            device_sort_rows(in->colidx, nnz, nbits, ka, pa, kb, pb, hist, hist_tmp, epi, s, ctx->rank_atomic);
        }
        launches += passes * (2 + scan_launches((uint64_t)rs_blocks(nnz) * kRadix));
        ingest_ptr_kernel<<<grid_for(N + 1, 256), 256, 0, s>>>(sorted_cols, nnz, N, res->rowptr);
        launches++;
    }
    finish_csr(res, ev, nnz, s);
    *st = osp_transpose_stats_t{};
    st->nnz = nnz;
    st->path = path;
    st->passes = passes;
    st->launches = launches;
    st->ms_total = res->info.ms_total;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] transpose M=%llu N=%llu nnz=%llu path=%u passes=%u launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, path, passes, launches, st->ms_total,
                (unsigned long long)ctx->malloc_calls);
}

// ---- a CSR result and dense vectors: reduce, apply, vertex select (osp_vector.h) ----
// R over every segment of (ptr, vals) into out[0, nseg): the short segments by a wave each, the long ones block by block
// into a pool buffer whose segments (one per long segment) are the next level's input.  nent: an upper bound of the level's
// entries.  One read-back per level that can hold a long segment (the number of long segments).  map: where a segment's
// result goes in out (null: at its own number).
template <class T, int OP>
static void reduce_segments(Scratch &sc, hipStream_t s, const int64_t *ptr, const T *vals, uint64_t nseg, uint64_t nent, T *out,
                            uint64_t &long_segments, uint32_t &launches, const uint32_t *map = nullptr) {
    for (int level = 0;; level++) {
        reduce_short_kernel<T, OP><<<grid_for(nseg, kReduceWaves), kReduceWaves * kWave, 0, s>>>(ptr, vals, nseg, map, out);
        launches++;
        if (nent <= kReduceBlock) return;   // (no segment can be long)
        unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(MCL_COUNTERS);
        zero_async(s, {{counters, MCL_COUNTERS * sizeof(uint64_t)}});
        uint32_t *long_segs = sc.get<uint32_t>(nent / ((uint64_t)kReduceBlock + 1) + 1);
        mcl_classify_kernel<<<grid_for(nseg, 256), 256, 0, s>>>(ptr, nseg, kReduceBlock, long_segs, counters);
        launches += 2;
        const uint64_t n_long = d2h((const uint64_t *)counters + MCL_NLONG, s);
        if (level == 0) long_segments = n_long;
        if (!n_long) return;
        // the long segments' blocks: sum ceil(m / block) <= nent / block + n_long, the exact number stays on the device
        const uint64_t max_blocks = nent / kReduceBlock + n_long;
        uint32_t *nblk = sc.get<uint32_t>(n_long + 1), *next_map = sc.get<uint32_t>(n_long);
        int64_t *blkptr = sc.get<int64_t>(n_long + 1);
        uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(n_long + 1));
        T *partial = sc.get<T>(max_blocks);
        reduce_long_setup_kernel<<<grid_for(n_long, 256), 256, 0, s>>>(ptr, long_segs, n_long, map, nblk, next_map);
        launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{nblk}, n_long, (uint64_t *)blkptr, tmp, s);
        reduce_blocks_kernel<T, OP><<<grid_for(max_blocks, kReduceWaves), kReduceWaves * kWave, 0, s>>>(ptr, vals, long_segs, blkptr, n_long, partial);
        launches++;
        ptr = blkptr;
        vals = partial;
        nseg = n_long;
        nent = max_blocks;
        map = next_map;
    }
}

template <class T>
static void reduce_impl(Context *ctx, const Result *in, int axis, int op, void *out_vec, osp_memspace_t space, osp_vector_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const uint64_t nout = axis == OSP_AXIS_ROWS ? M : N;
    uint64_t long_segments = 0;
    uint32_t launches = 0;
    // (the vector is formed in a pool buffer and copied out last: a call that fails leaves out_vec as it was)
    T *out = sc.get<T>(nout);
    const T inf = std::numeric_limits<T>::infinity();
    const T id = op == OSP_REDUCE_MIN ? inf : op == OSP_REDUCE_MAX ? -inf : T(0);
    std::vector<T> ids;
    if (nout && nnz) {
        const int64_t *ptr = in->rowptr;
        const T *vals = (const T *)in->vals;
        if (axis == OSP_AXIS_COLS) {
            // the column-major view: entries of one column keep ascending row order (its kernels are not counted below)
            int64_t *vptr;
            uint32_t *vidx;
            T *vvals;
            masked_view<T>(ctx, sc, M, N, nnz, in->rowptr, in->colidx, vals, &vptr, &vidx, &vvals);
            ptr = vptr;
            vals = vvals;
        }
        if (op == OSP_REDUCE_COUNT) {
            unsigned long long *counter = (unsigned long long *)sc.get<uint64_t>(1);
            zero_async(s, {{counter, sizeof(uint64_t)}});
            reduce_count_kernel<T><<<grid_for(nout, 256), 256, 0, s>>>(ptr, nout, out, counter);
            launches = 2;
            long_segments = d2h((const uint64_t *)counter, s);
        } else if (op == OSP_REDUCE_PLUS) {
            reduce_segments<T, RED_PLUS>(sc, s, ptr, vals, nout, nnz, out, long_segments, launches);
        } else if (op == OSP_REDUCE_MIN) {
            reduce_segments<T, RED_MIN>(sc, s, ptr, vals, nout, nnz, out, long_segments, launches);
        } else {
            reduce_segments<T, RED_MAX>(sc, s, ptr, vals, nout, nnz, out, long_segments, launches);
        }
    } else if (nout) {
        ids.assign(nout, id);   // every segment is empty: no kernel
    }
    OSP_HIP(hipEventRecord(ev.b, s));
    OSP_HIP(hipStreamSynchronize(s));
    OSP_HIP(hipGetLastError());
    if (nout) {
        if (!ids.empty()) {
            if (space == OSP_DEVICE) copy_h2d(out_vec, ids.data(), nout * sizeof(T), s);
            else memcpy(out_vec, ids.data(), nout * sizeof(T));
        } else if (space == OSP_DEVICE) {
            OSP_HIP(hipMemcpyAsync(out_vec, out, nout * sizeof(T), hipMemcpyDeviceToDevice, s));
        } else {
            copy_d2h(out_vec, out, nout * sizeof(T), s);
        }
        OSP_HIP(hipStreamSynchronize(s));
    }
    *st = osp_vector_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = nout;
    st->long_segments = long_segments;
    st->ms_total = ev.ms();
    st->launches = launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] reduce axis=%d op=%d M=%llu N=%llu nnz=%llu long=%llu launches=%u %.3f ms\n", axis, op, (unsigned long long)M,
                (unsigned long long)N, (unsigned long long)nnz, (unsigned long long)long_segments, launches, st->ms_total);
}

// ---- a CSR result times a dense vector under a semiring (osp_mxv.h) ----
// body(integral_constant ADD, integral_constant MUL) for the RED_* value `add` and the EW_* value `mul` (PLUS .. SECOND)
template <int ADD, int MUL = 0, class F>
static void mxv_with_mul(int mul, F &&body) {
    if constexpr (MUL <= EW_SECOND) {
        if (mul == MUL) body(std::integral_constant<int, ADD>{}, std::integral_constant<int, MUL>{});
        else mxv_with_mul<ADD, MUL + 1>(mul, body);
    }
}
template <class F>
static void mxv_with_ops(int add, int mul, F &&body) {
    if (add == RED_PLUS) mxv_with_mul<RED_PLUS>(mul, body);
    else if (add == RED_MIN) mxv_with_mul<RED_MIN>(mul, body);
    else mxv_with_mul<RED_MAX>(mul, body);
}

// log2 of the lanes a packed row gets.  OSP_MXV_GROUP = 4, 8, 16, 32 or 64 forces it (any other value: automatic).
// Automatic: the smallest g of at least the mean row length, the fastest of the five on the R-MAT adjacency that was measured
// (by 2-4 % over g = 64, MEASUREMENTS.md section 0l; means below 4 and other distributions: not measured).
static uint32_t mxv_group_log2(uint64_t M, uint64_t nnz) {
    const uint64_t forced = env_u64("OSP_MXV_GROUP", 0);
    for (uint32_t lg = 2; lg <= 6; lg++)
        if (forced == (1ull << lg)) return lg;
    uint32_t lg = 2;
    while (lg < 6 && (M << lg) < nnz) lg++;
    return lg;
}

template <class T>
static void mxv_impl(Context *ctx, const Result *in, const osp_semiring_t &sr, const void *x_in, void *y_out, osp_memspace_t space,
                     osp_mxv_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const int add = sr.add == OSP_EWISE_PLUS ? RED_PLUS : sr.add == OSP_EWISE_MIN ? RED_MIN : RED_MAX;
    const uint32_t lg = mxv_group_log2(M, nnz);
    uint64_t long_segments = 0;
    uint32_t launches = 0;
    // (the vector is formed in a pool buffer and copied out last: x may be y, and a call that fails leaves y as it was)
    T *out = sc.get<T>(M);
    std::vector<T> ids;
    if (M && nnz) {
        const T *x = sr.mul == OSP_EWISE_FIRST ? nullptr : to_device(sc, (const T *)x_in, N, space, s);
        const int64_t *rowptr = in->rowptr;
        const uint32_t *col = in->colidx;
        const T *vals = (const T *)in->vals;
        mxv_with_ops(add, sr.mul, [&](auto a, auto m) {
            constexpr int ADD = decltype(a)::value, MUL = decltype(m)::value;
            const uint64_t waves = (M + (kWave >> lg) - 1) >> (6 - lg);
            mxv_rows_kernel<T, ADD, MUL><<<grid_for(waves, kReduceWaves), kReduceWaves * kWave, 0, s>>>(rowptr, col, vals, x, M, lg, out);
            launches++;
            if (nnz <= kReduceBlock) return;   // (no row can be long)
            // the long rows, listed and cut into blocks as reduce_segments lists and cuts a level's long segments
            unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(MCL_COUNTERS);
            zero_async(s, {{counters, MCL_COUNTERS * sizeof(uint64_t)}});
            uint32_t *long_rows = sc.get<uint32_t>(nnz / ((uint64_t)kReduceBlock + 1) + 1);
            mcl_classify_kernel<<<grid_for(M, 256), 256, 0, s>>>(rowptr, M, kReduceBlock, long_rows, counters);
            launches += 2;
            const uint64_t n_long = d2h((const uint64_t *)counters + MCL_NLONG, s);
            long_segments = n_long;
            if (!n_long) return;
            const uint64_t max_blocks = nnz / kReduceBlock + n_long;
            uint32_t *nblk = sc.get<uint32_t>(n_long + 1), *map = sc.get<uint32_t>(n_long);
            int64_t *blkptr = sc.get<int64_t>(n_long + 1);
            uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(n_long + 1));
            T *partial = sc.get<T>(max_blocks);
            reduce_long_setup_kernel<<<grid_for(n_long, 256), 256, 0, s>>>(rowptr, long_rows, n_long, nullptr, nblk, map);
            launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{nblk}, n_long, (uint64_t *)blkptr, tmp, s);
            mxv_blocks_kernel<T, ADD, MUL><<<grid_for(max_blocks, kReduceWaves), kReduceWaves * kWave, 0, s>>>(rowptr, col, vals, x, long_rows, blkptr,
                                                                                                               n_long, partial);
            launches++;
            // the blocks' results are plain values: every further level is osp_csr_reduce's
            uint64_t deeper = 0;
            reduce_segments<T, ADD>(sc, s, blkptr, partial, n_long, max_blocks, out, deeper, launches, map);
        });
    } else if (M) {
        const T inf = std::numeric_limits<T>::infinity();
        ids.assign(M, add == RED_MIN ? inf : add == RED_MAX ? -inf : T(0));   // every row is empty: no kernel
    }
    OSP_HIP(hipEventRecord(ev.b, s));
    OSP_HIP(hipStreamSynchronize(s));
    OSP_HIP(hipGetLastError());
    if (M) {
        if (!ids.empty()) {
            if (space == OSP_DEVICE) copy_h2d(y_out, ids.data(), M * sizeof(T), s);
            else memcpy(y_out, ids.data(), M * sizeof(T));
        } else if (space == OSP_DEVICE) {
            OSP_HIP(hipMemcpyAsync(y_out, out, M * sizeof(T), hipMemcpyDeviceToDevice, s));
        } else {
            copy_d2h(y_out, out, M * sizeof(T), s);
        }
        OSP_HIP(hipStreamSynchronize(s));
    }
    *st = osp_mxv_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = M;
    st->long_segments = long_segments;
    st->group = 1u << lg;
    st->launches = launches;
    st->ms_total = ev.ms();
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] mxv add=%d mul=%d M=%llu N=%llu nnz=%llu group=%u long=%llu launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, 1u << lg, (unsigned long long)long_segments,
                launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

template <class T, int OP = 0>
static void launch_apply_rows(int op, hipStream_t s, const Result *in, const ValueBits<T> *src, const ValueBits<T> *x, Result *res) {
    if constexpr (OP < EW_OPS) {
        if (OP != EW_FIRST && op == OP)
            apply_rows_kernel<T, OP == EW_FIRST ? EW_SECOND : OP><<<grid_for(in->info.nnz_c, (unsigned)kCompactChunk), kCompactThreads, 0, s>>>(
                in->rowptr, in->colidx, in->info.M, in->info.nnz_c, src, x, (ValueBits<T> *)res->vals);
        else launch_apply_rows<T, OP + 1>(op, s, in, src, x, res);
    }
}
template <class T, int OP = 0>
static void launch_apply_cols(int op, hipStream_t s, const Result *in, const ValueBits<T> *src, const ValueBits<T> *y, Result *res) {
    if constexpr (OP < EW_OPS) {
        if (OP != EW_FIRST && op == OP)
            apply_cols_kernel<T, OP == EW_FIRST ? EW_SECOND : OP><<<grid_for(in->info.nnz_c, 256), 256, 0, s>>>(in->colidx, in->info.nnz_c, src, y,
                                                                                                             (ValueBits<T> *)res->vals);
        else launch_apply_cols<T, OP + 1>(op, s, in, src, y, res);
    }
}

template <class T>
static void apply_vectors_impl(Context *ctx, const Result *in, Result *res, const osp_vector_apply_t &ap, const void *x_in, const void *y_in,
                               osp_memspace_t space, osp_vector_stats_t *st) {
    typedef ValueBits<T> V;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    res->info = in->info;
    uint32_t launches = 0;
    if (M == 0 || nnz == 0) {
        empty_result<T>(res, M, s);
    } else {
        const bool rows = ap.row_op != OSP_VECTOR_NONE, cols = ap.col_op != OSP_VECTOR_NONE;
        const V *x = rows ? to_device(sc, (const V *)x_in, M, space, s) : nullptr;
        const V *y = cols ? to_device(sc, (const V *)y_in, N, space, s) : nullptr;
        alloc_rowptr(res, M);
        OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        alloc_entries<T>(res, nnz);
        OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        // one launch per side, the second in place on out's values
        const V *src = (const V *)in->vals;
        if (rows) {
            launch_apply_rows<T>(ap.row_op, s, in, src, x, res);
            src = (const V *)res->vals;
            launches++;
        }
        if (cols) {
            launch_apply_cols<T>(ap.col_op, s, in, src, y, res);
            launches++;
        }
    }
    finish_csr(res, ev, nnz, s);
    *st = osp_vector_stats_t{};
    st->nnz_in = st->nnz_out = nnz;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] apply_vectors row_op=%d col_op=%d M=%llu nnz=%llu launches=%u %.3f ms\n", ap.row_op, ap.col_op, (unsigned long long)M,
                (unsigned long long)nnz, launches, st->ms_total);
}

template <class T>
static void select_vertices_impl(Context *ctx, const Result *in, Result *res, const uint8_t *keep_rows_in, const uint8_t *keep_cols_in,
                                 osp_memspace_t space, osp_vector_stats_t *st) {
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz_in = in->info.nnz_c;
    res->info = in->info;
    const uint8_t *kr = keep_rows_in && nnz_in ? to_device(sc, keep_rows_in, M, space, s) : nullptr;
    const uint8_t *kc = keep_cols_in && nnz_in ? to_device(sc, keep_cols_in, N, space, s) : nullptr;
    const Compacted c = compact_by_bits<T>(sc, in, res, s, [&](unsigned nchunks, uint64_t *bits) {
        const auto flag = kr && kc ? vertex_flag_kernel<true, true> : kr ? vertex_flag_kernel<true, false> : vertex_flag_kernel<false, true>;
        flag<<<nchunks, kCompactThreads, 0, s>>>(in->rowptr, in->colidx, M, nnz_in, kr, kc, bits);
    });
    finish_csr(res, ev, c.nnz, s);
    *st = osp_vector_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = c.launches;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] select_vertices rows=%d cols=%d M=%llu nnz %llu -> %llu launches=%u %.3f ms\n", kr != nullptr, kc != nullptr,
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)c.nnz, c.launches, st->ms_total);
}

// ---- the submatrix in(rows, cols), renumbered (osp_extract.h) ----
static void check_extract_lists(uint32_t bad) {
    if (bad & kExtractBadRow) throw Error(OSP_ERR_ARG, "extract: a row index is not below the rows of in");
    if (bad & kExtractBadCol) throw Error(OSP_ERR_ARG, "extract: the columns are not strictly ascending and below the columns of in");
}

template <class T>
static void extract_impl(Context *ctx, const Result *in, Result *res, const osp_extract_t &ex, osp_extract_stats_t *st) {
    typedef ValueBits<T> V;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = in->info.M, N = in->info.N, nnz_in = in->info.nnz_c;
    const bool has_rows = ex.rows != nullptr, has_cols = ex.cols != nullptr;
    const uint64_t m = has_rows ? ex.n_rows : M, n = has_cols ? ex.n_cols : N;
    const osp_memspace_t space = (osp_memspace_t)ex.space;
    res->info = in->info;
    res->info.M = m; res->info.N = n;
    res->info.row_begin = 0; res->info.row_end = m;
    uint64_t nnz_g = has_rows ? 0 : nnz_in, nnz_out = 0;
    uint32_t launches = 0, readbacks = 0;
    if (nnz_in == 0 || m == 0 || n == 0) {
        if (has_rows) nnz_g = 0;
        empty_result<T>(res, m, s);
    } else if (!has_rows && !has_cols) {
        copy_csr<T>(in, res, s);
        nnz_out = nnz_in;
    } else {
        // (pool buffers are recycled, and OSP_POISON fills them: the error word and the bitmap are zeroed on every call)
        const uint64_t nwc = (N + 63) / 64;
        uint32_t *err = sc.get<uint32_t>(1);
        uint64_t *colbits = has_cols ? sc.get<uint64_t>(nwc) : nullptr;
        uint32_t *cpos = has_cols ? sc.get<uint32_t>(nwc + 1) : nullptr;   // (ranks of columns: below n <= 2^32 - 1)
        zero_async(s, {{err, sizeof(uint32_t)}, {colbits, has_cols ? nwc * sizeof(uint64_t) : 0}});
        launches++;
        const uint32_t *rows = nullptr;
        uint32_t *dense = nullptr;
        uint64_t *g = nullptr;   // the gathered row pointer; without a column list it IS out's row pointer
        if (has_rows) {
            rows = to_device(sc, ex.rows, m, space, s);
            uint32_t *len = sc.get<uint32_t>(m);
            uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(m));
            if (has_cols) g = sc.get<uint64_t>(m + 1);
            else { alloc_rowptr(res, m); g = (uint64_t *)res->rowptr; }
            extract_len_kernel<<<grid_for(m, 256), 256, 0, s>>>(rows, m, in->rowptr, M, len, err);
            launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{len}, m, g, tmp, s);
        }
        if (has_cols) {
            const uint32_t *cols = to_device(sc, ex.cols, n, space, s);
            uint32_t *tmp = sc.get<uint32_t>(scan_scratch_entries(nwc));
            if (env_is("OSP_EXTRACT_DENSE_MAP", "1")) dense = sc.get<uint32_t>(N);
            extract_colmap_kernel<<<grid_for(n, 256), 256, 0, s>>>(cols, n, N, (unsigned long long *)colbits, dense, err);
            launches += 1 + device_exclusive_scan<LoadPopc64, uint32_t>(LoadPopc64{colbits}, nwc, cpos, tmp, s);
        }
        uint32_t bad = 0;
        if (has_rows) {   // the first read-back: nothing an index decides is launched before the lists are known to be good
            Gather first(s);
            first.add(&bad, (const uint32_t *)err);
            first.add(&nnz_g, (const uint64_t *)g + m);
            first.wait();
            readbacks++;
            check_extract_lists(bad);
            if (nnz_g >= 0xffffffffull) throw Error(OSP_ERR_ARG, "extract: gathered rows of >= 2^32 - 1 non-zeros are not supported");
        }
        const int64_t *gp = has_rows ? (const int64_t *)g : in->rowptr;
        const unsigned nchunks = grid_for(nnz_g, (unsigned)kCompactChunk);
        if (nnz_g == 0) {
            if (has_cols) empty_result<T>(res, m, s);
            else alloc_entries<T>(res, 0);   // (g, all zeros, is the row pointer)
        } else if (!has_cols) {
            nnz_out = nnz_g;
            alloc_entries<T>(res, nnz_out);
            extract_write_kernel<V, true, false><<<nchunks, kCompactThreads, 0, s>>>(gp, rows, in->rowptr, in->colidx, (const V *)in->vals, m, nnz_g, nullptr,
                                                                                      nullptr, nullptr, nullptr, nullptr, res->colidx, (V *)res->vals);
            launches++;
        } else {
            alloc_rowptr(res, m);
            // (without a row list the verdicts need no index of the caller's as an address -- a bad column set no bit -- so the
            // error word travels with the one read-back of the scan)
            std::function<void(Gather &)> more;
            if (!has_rows) more = [&](Gather &ga) { ga.add(&bad, (const uint32_t *)err); };
            const BitScan b = flag_and_scan(sc, nnz_g, s, [&](unsigned grid, uint64_t *bits) {
                const auto flag = has_rows ? extract_flag_kernel<true> : extract_flag_kernel<false>;
                flag<<<grid, kCompactThreads, 0, s>>>(gp, rows, in->rowptr, in->colidx, m, nnz_g, colbits, bits);
            }, more);
            readbacks++;
            check_extract_lists(bad);
            launches += b.launches;
            nnz_out = b.count;
            alloc_entries<T>(res, nnz_out);
            compact_rowptr_kernel<<<grid_for(m + 1, 256), 256, 0, s>>>(gp, m, b.bits, b.pos, res->rowptr);
            launches++;
            if (nnz_out) {
                const auto write = has_rows ? extract_write_kernel<V, true, true> : extract_write_kernel<V, false, true>;
                write<<<nchunks, kCompactThreads, 0, s>>>(gp, rows, in->rowptr, in->colidx, (const V *)in->vals, m, nnz_g, b.bits, b.pos, colbits, cpos,
                                                          dense, res->colidx, (V *)res->vals);
                launches++;
            }
        }
    }
    finish_csr(res, ev, nnz_out, s);
    *st = osp_extract_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_gathered = nnz_g;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] extract rows=%d cols=%d %llu x %llu of %llu x %llu nnz %llu -> %llu -> %llu launches=%u readbacks=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                has_rows, has_cols, (unsigned long long)m, (unsigned long long)n, (unsigned long long)M, (unsigned long long)N,
                (unsigned long long)nnz_in, (unsigned long long)nnz_g, (unsigned long long)nnz_out, launches, readbacks, st->ms_total,
                (unsigned long long)ctx->malloc_calls);
}

// ---- a CSR result from a COO list, repeats combined in list order (osp_build.h) ----
template <class T, int OP, bool VALS>
static void launch_build_write(unsigned grid, hipStream_t s, const uint32_t *col, const uint32_t *perm, const ValueBits<T> *vals, uint64_t nnz,
                               const BitScan &h, Result *res, unsigned long long *n_long) {
    build_write_kernel<T, OP, VALS><<<grid, kCompactThreads, 0, s>>>(col, perm, vals, nnz, h.count, h.bits, h.pos, res->colidx, (ValueBits<T> *)res->vals,
                                                                     n_long);
}

template <class T>
static void build_impl(Context *ctx, Result *res, const osp_build_t &b, osp_build_stats_t *st) {
    typedef ValueBits<T> V;
    hipStream_t s = ctx->stream;
    Scratch sc(ctx);
    EventPair ev;
    OSP_HIP(hipEventRecord(ev.a, s));
    const uint64_t M = b.M, N = b.N, nnz = b.nnz;
    const osp_memspace_t space = (osp_memspace_t)b.space;
    const int dup = b.dup;
    res->info = osp_result_info_t{};   // every field the build does not name stays 0
    res->info.dtype = res->dtype;
    note_variants(ctx, res);
    res->info.M = M; res->info.N = N;
    res->info.row_begin = 0; res->info.row_end = M;
    uint64_t nnz_out = 0, long_runs = 0;
    uint32_t launches = 0, readbacks = 0;
    if (nnz == 0 || M == 0 || N == 0) {
        empty_result<T>(res, M, s);
    } else {
        const bool has_vals = b.vals != nullptr && dup != DUP_COUNT;   // (COUNT reads no value: none is copied either)
        const bool folds = has_vals && (dup == DUP_PLUS || dup == DUP_MIN || dup == DUP_MAX);
        const uint32_t *rows = to_device(sc, b.rows, nnz, space, s), *cols = to_device(sc, b.cols, nnz, space, s);
        const V *vals = has_vals ? to_device(sc, (const V *)b.vals, nnz, space, s) : nullptr;
        uint32_t *ka = sc.get<uint32_t>(nnz), *pa = sc.get<uint32_t>(nnz), *kb = sc.get<uint32_t>(nnz), *pb = sc.get<uint32_t>(nnz);
        uint32_t *k1 = sc.get<uint32_t>(nnz), *perm1 = sc.get<uint32_t>(nnz), *k2 = sc.get<uint32_t>(nnz);
        uint32_t *row_sorted = sc.get<uint32_t>(nnz), *perm = sc.get<uint32_t>(nnz), *col_sorted = k1;   // (k1 is free after the second sort)
        uint32_t *hist = sc.get<uint32_t>(rs_hist_entries(nnz));
        uint32_t *hist_tmp = sc.get<uint32_t>(scan_scratch_entries(rs_hist_entries(nnz)));
        int64_t *sptr = sc.get<int64_t>(M + 1);   // the sorted list's row pointer
        // (pool buffers are recycled, and OSP_POISON fills them: the error word and the counter are zeroed on every call)
        uint32_t *err = sc.get<uint32_t>(2);
        unsigned long long *n_long = sc.get<unsigned long long>(1);
        zero_async(s, {{err, sizeof(uint32_t)}, {n_long, sizeof(unsigned long long)}});
        launches++;
        // stable LSD, as coo_to_compressed_device: by column first, then by row
        const int cbits = std::max(1, bits_for(N)), rbits = std::max(1, bits_for(M));
        device_sort_rows<RsStoreEpilogue>(cols, nnz, cbits, ka, pa, kb, pb, hist, hist_tmp, RsStoreEpilogue{k1, perm1}, s, ctx->rank_atomic);
        ingest_gather_u32_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(rows, perm1, nnz, k2);
        device_sort_rows<RsStoreEpilogue>(k2, nnz, rbits, ka, pa, kb, pb, hist, hist_tmp, RsStoreEpilogue{row_sorted, perm}, s, ctx->rank_atomic,
                                          perm1);
        ingest_gather_u32_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(cols, perm, nnz, col_sorted);
        ingest_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(row_sorted, nnz, M, sptr);
        launches += (uint32_t)((cbits + 7) / 8 + (rbits + 7) / 8) * (2 + scan_launches((uint64_t)rs_blocks(nnz) * kRadix)) + 3;
        // the call's read-back: the number of runs, with the error word -- nothing of out exists before the list is known to be good
        uint32_t bad = 0;
        const BitScan h = flag_and_scan(sc, nnz, s, [&](unsigned grid, uint64_t *bits) {
            build_heads_kernel<<<grid, kCompactThreads, 0, s>>>(row_sorted, col_sorted, nnz, M, N, bits, err);
        }, [&](Gather &ga) { ga.add(&bad, (const uint32_t *)err); });
        readbacks++;
        launches += h.launches;
        if (bad) throw Error(OSP_ERR_RANGE, "build: an index of the list is outside its dimension");
        if (dup == DUP_ERROR && h.count < nnz) throw Error(OSP_ERR_DUPLICATE, "build: duplicate coordinate (dup = OSP_DUP_ERROR)");
        nnz_out = h.count;
        alloc_rowptr(res, M);
        alloc_entries<T>(res, nnz_out);
        compact_rowptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(sptr, M, h.bits, h.pos, res->rowptr);
        const unsigned grid = grid_for(nnz, (unsigned)kCompactChunk);
        if (has_vals) {
            switch (dup) {
                case DUP_PLUS: launch_build_write<T, DUP_PLUS, true>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                case DUP_MIN: launch_build_write<T, DUP_MIN, true>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                case DUP_MAX: launch_build_write<T, DUP_MAX, true>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                case DUP_LAST: launch_build_write<T, DUP_LAST, true>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                default: launch_build_write<T, DUP_FIRST, true>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;   // FIRST, ERROR
            }
        } else {
            switch (dup) {
                case DUP_PLUS: launch_build_write<T, DUP_PLUS, false>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                case DUP_COUNT: launch_build_write<T, DUP_COUNT, false>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;
                default: launch_build_write<T, DUP_FIRST, false>(grid, s, col_sorted, perm, vals, nnz, h, res, n_long); break;   // every value is 1
            }
        }
        launches += 2;
        if (folds && nnz_out < nnz) {   // only then can a wave have folded a run
            Gather last(s);
            last.add(&long_runs, (const uint64_t *)n_long);
            last.wait();
            readbacks++;
        }
    }
    finish_csr(res, ev, nnz_out, s);
    *st = osp_build_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = nnz_out;
    st->long_runs = long_runs;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (getenv("OSP_VERBOSE"))
        fprintf(stderr, "[osp] build dup=%d vals=%d %llu x %llu nnz %llu -> %llu long_runs=%llu launches=%u readbacks=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                dup, b.vals != nullptr, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, (unsigned long long)nnz_out,
                (unsigned long long)long_runs, launches, readbacks, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

static void destroy_result(Result *r) {
    if (!r) return;
    if (r->ctx) {
        r->ctx->release(r->rowptr);
        r->ctx->release(r->colidx);
        r->ctx->release(r->vals);
    }
    delete r;
}

// ---- what the entry points share ----
static void check_dtype(int dtype) {
    if (dtype != OSP_F32 && dtype != OSP_F64) throw Error(OSP_ERR_ARG, "dtype must be OSP_F32 or OSP_F64");
}
static void check_space(int space) {
    if (space != OSP_HOST && space != OSP_DEVICE) throw Error(OSP_ERR_ARG, "bad memory space");
}
static void check_dims(uint64_t M, uint64_t K, uint64_t N) {   // (K = 0: no inner dimension)
    if (M >= 0xffffffffull || N > 0xffffffffull || K >= 0xffffffffull) throw Error(OSP_ERR_ARG, "dimension exceeds the u32 index type");
}
static osp_config_t config_or_default(const osp_config_t *cfg) {
    osp_config_t c;
    if (cfg) c = *cfg; else osp_config_default(&c);
    return c;
}
// body(T{}) with T the value type of a checked dtype
template <class F>
static void with_type(int dtype, F &&body) {
    if (dtype == OSP_F32) body(float{});
    else body(double{});
}
// Runs `body` on ctx's device.  When it throws, the stream is drained before the exception travels on: no buffer goes back
// to the pool while work queued on it may still use it.
template <class F>
static void on_device(Context *ctx, F &&body) {
    try {
        OSP_HIP(hipSetDevice(ctx->device));
        body();
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        throw;
    }
}
// The frame of an entry point that makes a result: body(T{}, res) fills a new result on ctx's device, T the value type of
// `dtype`.  *out gets it when body returns; when body throws, it is released (after the stream is drained) and *out is left
// as it was.
template <class F>
static int new_result(Context *ctx, int dtype, osp_result_t *out, F &&body) {
    std::unique_ptr<Result, void (*)(Result *)> res(new Result, destroy_result);
    res->ctx = ctx;
    res->dtype = dtype;
    res->info.dtype = dtype;
    note_variants(ctx, res.get());
    on_device(ctx, [&] { with_type(dtype, [&](auto tag) { body(tag, res.get()); }); });
    *out = (osp_result_t)res.release();
    return OSP_OK;
}

}  // namespace osp

#include "osp_multi.h"

using namespace osp;

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" {

const char *osp_status_string(int st) {
    switch (st) {
        case OSP_OK: return "ok";
        case OSP_ERR_DIM: return "inner dimensions differ";
        case OSP_ERR_ARG: return "bad argument";
        case OSP_ERR_ALLOC: return "allocation failed";
        case OSP_ERR_HIP: return "HIP error";
        case OSP_ERR_IO: return "I/O error";
        case OSP_ERR_RANGE: return "index out of range";
        case OSP_ERR_CAPACITY: return "staging capacity exceeded";
        case OSP_ERR_UNSORTED: return "indices not ascending";
        case OSP_ERR_DUPLICATE: return "duplicate coordinate (233)";
        default: return "unknown status";
    }
}

void osp_config_default(osp_config_t *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->validate = 1;
}

static int context_create(int device, void *stream, bool own, osp_context_t *out) {
    if (!out) return fail(OSP_ERR_ARG, "null context pointer");
    return guard([&] {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw Error(OSP_ERR_HIP, "no HIP device visible: this library has no CPU path");
        if (device < 0 || device >= ndev) throw Error(OSP_ERR_ARG, "device ordinal out of range");
        OSP_HIP(hipSetDevice(device));
        hipDeviceProp_t prop;
        OSP_HIP(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            throw Error(OSP_ERR_HIP, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
        Context *c = new Context;
        c->device = device;
        c->cus = (uint32_t)prop.multiProcessorCount;
        if (own) { OSP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
        else c->stream = (hipStream_t)stream;
        try {
            // Which stable rank this context uses.  The atomic one needs a property of LDS atomics that is not documented, so
            // it is tested here on THIS device; when the test fails the context falls back to the ballot instantiations of the
            // same kernels (slower -- merge +20 % -- and just as exact) instead of refusing to work.
            const char *force = getenv("OSP_RANK");   // "ballot" | "atomic": debugging and tests/test_gpu_parity.py
            if (force && strcmp(force, "ballot") == 0) c->rank_atomic = false;
            else if (force && strcmp(force, "atomic") == 0) c->rank_atomic = true;
            if (c->rank_atomic) {
                Scratch sc(c);
                uint32_t *bad = sc.get<uint32_t>(1);
                OSP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
                rank_order_selftest_kernel<<<64, 256, 0, c->stream>>>(bad);
                if (d2h(bad, c->stream) != 0) {
                    c->rank_atomic = false;
                    if (getenv("OSP_VERBOSE")) fprintf(stderr, "[osp] LDS atomics do not return old values in lane order on this device: using ballot ranks\n");
                }
            }
            const char *fadd = getenv("OSP_DENSE_ADD");
            for (int wide = 0; wide < 2; wide++) {
                if (fadd && strcmp(fadd, "ballot") == 0) c->dense_atomic[wide] = false;
                else if (fadd && strcmp(fadd, "atomic") == 0) c->dense_atomic[wide] = true;
                if (!c->dense_atomic[wide]) continue;
                Scratch sc(c);
                uint32_t *bad = sc.get<uint32_t>(1);
                OSP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
                if (wide) fadd_order_selftest_kernel<double><<<64, 256, 0, c->stream>>>(bad);
                else fadd_order_selftest_kernel<float><<<64, 256, 0, c->stream>>>(bad);
                if (d2h(bad, c->stream) != 0) {
                    c->dense_atomic[wide] = false;
                    if (getenv("OSP_VERBOSE"))
                        fprintf(stderr, "[osp] LDS %s atomics do not add in lane order (or flush subnormals) on this device: dense segments by ballot ranks\n",
                                wide ? "f64" : "f32");
                }
            }
        } catch (...) {
            c->trim();
            if (c->own_stream) (void)hipStreamDestroy(c->stream);
            delete c;
            throw;
        }
        *out = (osp_context_t)c;
        return OSP_OK;
    });
}
int osp_context_create(int device, osp_context_t *ctx) { return context_create(device, nullptr, true, ctx); }
int osp_context_create_on_stream(int device, void *hip_stream, osp_context_t *ctx) {
    return context_create(device, hip_stream, false, ctx);
}
int osp_context_trim(osp_context_t c) {
    if (!c) return fail(OSP_ERR_ARG, "null context");
    ((Context *)c)->trim();
    return OSP_OK;
}
int osp_context_alloc(osp_context_t c_, uint64_t bytes, void **device_ptr) {
    Context *c = (Context *)c_;
    if (!c || !device_ptr) return fail(OSP_ERR_ARG, "null argument");
    return guard([&] {
        OSP_HIP(hipSetDevice(c->device));
        *device_ptr = c->alloc((size_t)bytes);
        return OSP_OK;
    });
}
int osp_context_free(osp_context_t c_, void *device_ptr) {
    Context *c = (Context *)c_;
    if (!c) return fail(OSP_ERR_ARG, "null context");
    c->release(device_ptr);
    return OSP_OK;
}
int osp_context_destroy(osp_context_t c_) {
    Context *c = (Context *)c_;
    if (!c) return OSP_OK;
    if (c->sibling) c->sibling->sibling = nullptr;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->trim();
    for (auto &kv : c->live) (void)hipFree(kv.first);
    c->drop_aux();
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return OSP_OK;
}

int osp_spgemm_csc_csr(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N,
                       const int64_t *a_colptr, const uint32_t *a_rowidx, const void *a_vals,
                       const int64_t *b_rowptr, const uint32_t *b_colidx, const void *b_vals,
                       osp_memspace_t space, const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if (!a_colptr || !b_rowptr) return fail(OSP_ERR_ARG, "null pointer array");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, K, N);
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            spgemm_impl<T>(ctx, res, M, K, N, a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals, space, cfg);
        });
    });
}

int osp_spgemm_masked(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr,
                      const uint32_t *a_rowidx, const void *a_vals, const int64_t *b_rowptr, const uint32_t *b_colidx, const void *b_vals,
                      const int64_t *m_rowptr, const uint32_t *m_colidx, osp_memspace_t space, const osp_config_t *cfg_,
                      osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if (!a_colptr || !b_rowptr || !m_rowptr) return fail(OSP_ERR_ARG, "null pointer array");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, K, N);
        const osp_config_t cfg = config_or_default(cfg_);
        if (cfg.k_begin != 0 || cfg.k_end != 0) throw Error(OSP_ERR_ARG, "masked product: k_begin / k_end must be 0 / 0");
        if (cfg.row_shard_count > 1) throw Error(OSP_ERR_ARG, "masked product: row shards are not supported");
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            masked_impl<T>(ctx, res, M, K, N, a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals, m_rowptr,
                           m_colidx, space, cfg);
        });
    });
}

int osp_csr_inflate_prune(osp_result_t in_, const osp_mcl_step_t *step, int validate, osp_result_t *out, osp_mcl_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !step || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        if (!(step->power >= 1.0) || !(step->power < HUGE_VAL)) throw Error(OSP_ERR_ARG, "inflate_prune: power must be a finite number >= 1");
        if (!(step->threshold >= 0.0) || !(step->threshold < HUGE_VAL)) throw Error(OSP_ERR_ARG, "inflate_prune: threshold must be a finite number >= 0");
        for (uint32_t w : step->reserved)
            if (w) throw Error(OSP_ERR_ARG, "inflate_prune: reserved words must be 0");
        osp_mcl_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            inflate_prune_impl<decltype(tag)>(in->ctx, in, res, *step, validate, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_apply_mask(osp_result_t in_, uint64_t M, uint64_t N, const int64_t *m_rowptr, const uint32_t *m_colidx, osp_memspace_t space,
                       int complement, int validate, osp_result_t *out, osp_apply_mask_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !out || !m_rowptr) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(space);
        if (M != in->info.M || N != in->info.N) throw Error(OSP_ERR_ARG, "apply_mask: the mask's shape differs from the result's");
        osp_apply_mask_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            apply_mask_impl<decltype(tag)>(in->ctx, in, res, m_rowptr, m_colidx, space, complement, validate, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_select(osp_result_t in_, const osp_select_t *sel, osp_result_t *out, osp_select_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !sel || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        if (sel->op < OSP_SELECT_LT || sel->op > OSP_SELECT_OFFDIAG) throw Error(OSP_ERR_ARG, "select: op is not one of osp_select_op_t");
        for (uint32_t w : sel->reserved)
            if (w) throw Error(OSP_ERR_ARG, "select: reserved words must be 0");
        osp_select_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            select_impl<decltype(tag)>(in->ctx, in, res, *sel, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_ewise(osp_result_t a_, osp_result_t b_, const osp_ewise_t *ew, osp_result_t *out, osp_ewise_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_;
    if (!a || !b || !ew || !out) return fail(OSP_ERR_ARG, "null argument");
    if (a->partials || b->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        if (ew->mode != OSP_EWISE_UNION && ew->mode != OSP_EWISE_INTERSECT) throw Error(OSP_ERR_ARG, "ewise: mode is not one of osp_ewise_mode_t");
        if (ew->op < OSP_EWISE_PLUS || ew->op > OSP_EWISE_DIV) throw Error(OSP_ERR_ARG, "ewise: op is not one of osp_ewise_op_t");
        if (ew->mode == OSP_EWISE_UNION && (ew->op == OSP_EWISE_MINUS || ew->op == OSP_EWISE_DIV))
            throw Error(OSP_ERR_ARG, "ewise: MINUS and DIV are not defined for a union (an entry of b alone would be copied as it is)");
        for (uint32_t w : ew->reserved)
            if (w) throw Error(OSP_ERR_ARG, "ewise: reserved words must be 0");
        if (a->ctx != b->ctx) throw Error(OSP_ERR_ARG, "ewise: the operands belong to different contexts");
        if (a->info.M != b->info.M || a->info.N != b->info.N) throw Error(OSP_ERR_ARG, "ewise: the operands' shapes differ");
        if (a->dtype != b->dtype) throw Error(OSP_ERR_ARG, "ewise: the operands' dtypes differ");
        if (a->info.nnz_c >= 0xffffffffull || b->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "ewise: operands with >= 2^32 - 1 non-zeros are not supported");
        osp_ewise_stats_t st{};
        const int rc = new_result(a->ctx, a->dtype, out, [&](auto tag, Result *res) {
            ewise_impl<decltype(tag)>(a->ctx, a, b, res, *ew, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_mxm(osp_result_t a_, osp_result_t b_, const osp_semiring_t *sr, osp_result_t *out, osp_mxm_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_;
    if (!a || !b || !sr || !out) return fail(OSP_ERR_ARG, "null argument");
    if (a->partials || b->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX && sr->add != OSP_EWISE_FIRST)
            throw Error(OSP_ERR_ARG, "mxm: add is not one of PLUS, MIN, MAX, FIRST");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "mxm: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        for (uint32_t w : sr->reserved)
            if (w) throw Error(OSP_ERR_ARG, "mxm: reserved words must be 0");
        if (a->ctx != b->ctx) throw Error(OSP_ERR_ARG, "mxm: the operands belong to different contexts");
        if (a->dtype != b->dtype) throw Error(OSP_ERR_ARG, "mxm: the operands' dtypes differ");
        if (a->info.nnz_c >= 0xffffffffull || b->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "mxm: operands with >= 2^32 - 1 non-zeros are not supported");
        if (a->info.N != b->info.M) throw Error(OSP_ERR_DIM, "mxm: a's N differs from b's M");
        osp_mxm_stats_t st{};
        const int rc = new_result(a->ctx, a->dtype, out, [&](auto tag, Result *res) {
            mxm_impl<decltype(tag)>(a->ctx, a, b, res, *sr, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_transpose(osp_result_t in_, const osp_transpose_t *tp, osp_result_t *out, osp_transpose_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        if (tp)
            for (uint32_t w : tp->reserved)
                if (w) throw Error(OSP_ERR_ARG, "transpose: reserved words must be 0");
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "transpose: an operand with >= 2^32 - 1 non-zeros is not supported");
        if (in->info.M > (1ull << 32)) throw Error(OSP_ERR_DIM, "transpose: a row index of in must fit a column of out");
        osp_transpose_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            transpose_impl<decltype(tag)>(in->ctx, in, res, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_reduce(osp_result_t in_, int axis, int op, void *out_vec, osp_memspace_t space, osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !out_vec) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(space);
        if (axis != OSP_AXIS_ROWS && axis != OSP_AXIS_COLS) throw Error(OSP_ERR_ARG, "reduce: axis is not one of osp_axis_t");
        if (op < OSP_REDUCE_PLUS || op > OSP_REDUCE_COUNT) throw Error(OSP_ERR_ARG, "reduce: op is not one of osp_reduce_op_t");
        if (axis == OSP_AXIS_COLS && in->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "reduce: the column axis does not support results with >= 2^32 - 1 non-zeros");
        osp_vector_stats_t st{};
        on_device(in->ctx, [&] { with_type(in->dtype, [&](auto tag) { reduce_impl<decltype(tag)>(in->ctx, in, axis, op, out_vec, space, &st); }); });
        if (stats) *stats = st;
        return (int)OSP_OK;
    });
}

int osp_csr_mxv(osp_result_t in_, const osp_semiring_t *sr, const void *x, void *y, osp_memspace_t space, osp_mxv_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !sr || !y) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(space);
        if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX) throw Error(OSP_ERR_ARG, "mxv: add is not one of PLUS, MIN, MAX");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "mxv: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        for (uint32_t w : sr->reserved)
            if (w) throw Error(OSP_ERR_ARG, "mxv: reserved words must be 0");
        if (!x && sr->mul != OSP_EWISE_FIRST) throw Error(OSP_ERR_ARG, "mxv: x may be null only when mul is FIRST");
        osp_mxv_stats_t st{};
        on_device(in->ctx, [&] { with_type(in->dtype, [&](auto tag) { mxv_impl<decltype(tag)>(in->ctx, in, *sr, x, y, space, &st); }); });
        if (stats) *stats = st;
        return (int)OSP_OK;
    });
}

int osp_csr_apply_vectors(osp_result_t in_, const osp_vector_apply_t *ap, const void *x_rows, const void *y_cols, osp_memspace_t space,
                          osp_result_t *out, osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !ap || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(space);
        for (int32_t o : {ap->row_op, ap->col_op})
            if (o != OSP_VECTOR_NONE && (o < OSP_EWISE_PLUS || o > OSP_EWISE_DIV || o == OSP_EWISE_FIRST))
                throw Error(OSP_ERR_ARG, "apply_vectors: an op is PLUS, TIMES, MINUS, DIV, MIN, MAX, SECOND or OSP_VECTOR_NONE");
        if (ap->row_op == OSP_VECTOR_NONE && ap->col_op == OSP_VECTOR_NONE) throw Error(OSP_ERR_ARG, "apply_vectors: both sides are OSP_VECTOR_NONE");
        for (uint32_t w : ap->reserved)
            if (w) throw Error(OSP_ERR_ARG, "apply_vectors: reserved words must be 0");
        if ((ap->row_op != OSP_VECTOR_NONE && !x_rows) || (ap->col_op != OSP_VECTOR_NONE && !y_cols))
            throw Error(OSP_ERR_ARG, "apply_vectors: a side with an op needs its vector");
        osp_vector_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            apply_vectors_impl<decltype(tag)>(in->ctx, in, res, *ap, x_rows, y_cols, space, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_select_vertices(osp_result_t in_, const uint8_t *keep_rows, const uint8_t *keep_cols, osp_memspace_t space, osp_result_t *out,
                            osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(space);
        if (!keep_rows && !keep_cols) throw Error(OSP_ERR_ARG, "select_vertices: keep_rows and keep_cols are both null");
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "select_vertices: results with >= 2^32 - 1 non-zeros are not supported");
        osp_vector_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            select_vertices_impl<decltype(tag)>(in->ctx, in, res, keep_rows, keep_cols, space, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_extract(osp_result_t in_, const osp_extract_t *ex, osp_result_t *out, osp_extract_stats_t *stats) {
    Result *in = (Result *)in_;
    if (!in || !ex || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(ex->space);
        for (uint32_t w : ex->reserved)
            if (w) throw Error(OSP_ERR_ARG, "extract: reserved words must be 0");
        check_dims(ex->rows ? ex->n_rows : 0, 0, ex->cols ? ex->n_cols : 0);
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "extract: results with >= 2^32 - 1 non-zeros are not supported");
        osp_extract_stats_t st{};
        const int rc = new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            extract_impl<decltype(tag)>(in->ctx, in, res, *ex, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_csr_build(osp_context_t ctx_, const osp_build_t *b, osp_result_t *out, osp_build_stats_t *stats) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !b || !out) return fail(OSP_ERR_ARG, "null argument");
    if (b->nnz && (!b->rows || !b->cols)) return fail(OSP_ERR_ARG, "build: null index list");
    return guard([&] {
        check_dtype(b->dtype); check_space(b->space);
        if (b->dup < 0 || b->dup >= DUP_OPS) throw Error(OSP_ERR_ARG, "build: dup must be an osp_dup_op_t");
        for (uint32_t w : b->reserved)
            if (w) throw Error(OSP_ERR_ARG, "build: reserved words must be 0");
        check_dims(b->M, 0, b->N);
        if (b->nnz >= 0xffffffffull) throw Error(OSP_ERR_ARG, "build: lists of >= 2^32 - 1 entries are not supported");
        osp_build_stats_t st{};
        const int rc = new_result(ctx, b->dtype, out, [&](auto tag, Result *res) {
            build_impl<decltype(tag)>(ctx, res, *b, &st);
        });
        if (stats) *stats = st;
        return rc;
    });
}

int osp_spgemm_csc_csr_aos(osp_context_t ctx_,osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, const uint64_t *a_pos,
                           const void *a_data, const uint64_t *b_pos, const void *b_data, osp_memspace_t space,
                           const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if (!a_pos || !b_pos) return fail(OSP_ERR_ARG, "null pointer array");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, K, N);
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            spgemm_aos_impl<decltype(tag)>(ctx, res, M, K, N, a_pos, a_data, b_pos, b_data, space, cfg);
        });
    });
}

int osp_spgemm_csc_csr_panels(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N,
                              const int64_t *a_colptr, const uint32_t *a_rowidx, const void *a_vals,
                              const int64_t *b_rowptr, const uint32_t *b_colidx, const void *b_vals,
                              osp_memspace_t space, const osp_config_t *cfg_, osp_panel_fn fn, void *user,
                              osp_result_info_t *info) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !fn) return fail(OSP_ERR_ARG, "null context or panel callback");
    if (!a_colptr || !b_rowptr) return fail(OSP_ERR_ARG, "null pointer array");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, K, N);
        const osp_config_t cfg = config_or_default(cfg_);
        const PanelSink sink{fn, user};
        osp_result_t r = nullptr;   // carries the counters only: no output arrays are attached in streaming mode
        new_result(ctx, dtype, &r, [&](auto tag, Result *res) {
            using T = decltype(tag);
            spgemm_impl<T>(ctx, res, M, K, N, a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals, space, cfg,
                           &sink);
            if (info) *info = res->info;
        });
        destroy_result((Result *)r);
        return OSP_OK;
    });
}

int osp_spgemm_coo(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, uint64_t nnz_a,
                   const uint32_t *a_rows, const uint32_t *a_cols, const void *a_vals, uint64_t nnz_b,
                   const uint32_t *b_rows, const uint32_t *b_cols, const void *b_vals, osp_memspace_t space,
                   const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if ((nnz_a && (!a_rows || !a_cols || !a_vals)) || (nnz_b && (!b_rows || !b_cols || !b_vals))) return fail(OSP_ERR_ARG, "null operand array");
    return guard([&] {
        check_dtype(dtype); check_space(space);
        if (M >= 0xffffffffull || N > 0xffffffffull || K >= 0xffffffffull || nnz_a >= 0xffffffffull || nnz_b >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "dimension or nnz exceeds the u32 index type");
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            spgemm_coo_impl<T>(ctx, res, M, K, N, nnz_a, a_rows, a_cols, (const T *)a_vals, nnz_b, b_rows, b_cols, (const T *)b_vals, space,
                               cfg);
        });
    });
}

int osp_merge_csr_parts(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t N, int nparts,
                        const int64_t *const *rowptrs, const uint32_t *const *colidxs,
                        const void *const *valss, osp_memspace_t space, const osp_config_t *cfg_,
                        osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result || !rowptrs || !colidxs || !valss) return fail(OSP_ERR_ARG, "null argument");
    if (nparts < 1) return fail(OSP_ERR_ARG, "nparts must be >= 1");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, 0, N);
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            merge_parts_impl<decltype(tag)>(ctx, res, M, N, nparts, rowptrs, colidxs, valss, space, cfg);
        });
    });
}

int osp_spgemm_partials(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr,
                        const uint32_t *a_rowidx, const void *a_vals, const int64_t *b_rowptr, const uint32_t *b_colidx,
                        const void *b_vals, osp_memspace_t space, const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if (!a_colptr || !b_rowptr) return fail(OSP_ERR_ARG, "null pointer array");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, K, N);
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            spgemm_impl<T>(ctx, res, M, K, N, a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals, space, cfg,
                           nullptr, true);
        });
    });
}

int osp_result_partials(osp_result_t r_, const int64_t **rowptr, const void **records) {
    Result *r = (Result *)r_;
    if (!r) return fail(OSP_ERR_ARG, "null result");
    if (!r->partials) return fail(OSP_ERR_ARG, "not a result of osp_spgemm_partials");
    if (rowptr) *rowptr = r->rowptr;
    if (records) *records = r->vals;
    return OSP_OK;
}

int osp_merge_record_parts(osp_context_t ctx_, osp_dtype_t dtype, uint64_t M, uint64_t N, int nparts, const int64_t *const *rowptrs,
                           const void *const *records, osp_memspace_t space, const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result || !rowptrs || !records) return fail(OSP_ERR_ARG, "null argument");
    if (nparts < 1) return fail(OSP_ERR_ARG, "nparts must be >= 1");
    return guard([&] {
        check_dtype(dtype); check_space(space); check_dims(M, 0, N);
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            merge_record_parts_impl<decltype(tag)>(ctx, res, M, N, nparts, rowptrs, records, space, cfg);
        });
    });
}

int osp_csr_bias_relu(osp_result_t in_, const void *bias, osp_memspace_t bias_space, int relu, osp_result_t *out) {
    Result *in = (Result *)in_;
    if (!in || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        check_space(bias_space);
        return new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {
            using T = decltype(tag);
            bias_relu_impl<T>(in->ctx, in, res, (const T *)bias, bias_space, relu);   // (res->info: in's, variants included)
        });
    });
}

int osp_result_coo_rows(osp_result_t r_, uint32_t *rows_device) {
    Result *r = (Result *)r_;
    if (!r || !rows_device) return fail(OSP_ERR_ARG, "null argument");
    if (r->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return guard([&] {
        OSP_HIP(hipSetDevice(r->ctx->device));
        const uint64_t M = r->info.M;
        if (M && r->info.nnz_c)
            csr_expand_rows_kernel<<<grid_for(M * kWave, 256), 256, 0, r->ctx->stream>>>(r->rowptr, M, rows_device);
        OSP_HIP(hipStreamSynchronize(r->ctx->stream));
        OSP_HIP(hipGetLastError());
        return OSP_OK;
    });
}

int osp_im2col_csc(osp_context_t ctx_, osp_dtype_t dtype, uint64_t N, uint64_t C, uint64_t H, uint64_t W, uint64_t nnz_x,
                   const uint32_t *x_rows, const uint32_t *x_cols, const void *x_vals, osp_memspace_t space,
                   const osp_conv2d_geometry_t *geom, int validate, uint64_t *nnz_a, int64_t *a_colptr, uint32_t *a_rowidx,
                   void *a_vals) {
    Context *ctx = (Context *)ctx_;
    (void)validate;   // the channel grouping checks x's ranges and duplicates in every case
    if (!ctx || !nnz_a) return fail(OSP_ERR_ARG, "null context or nnz_a pointer");
    if (nnz_x && (!x_rows || !x_cols || !x_vals)) return fail(OSP_ERR_ARG, "null operand array");
    return guard([&] {
        check_dtype(dtype); check_space(space);
        if (nnz_x >= 0xffffffffull) throw Error(OSP_ERR_ARG, "nnz exceeds the u32 index type");
        const bool fill = a_colptr || a_rowidx || a_vals;
        if (fill && !a_colptr) throw Error(OSP_ERR_ARG, "a_colptr is null but other output arrays are not");
        on_device(ctx, [&] {
            const ConvGeom g = conv_geometry(N, C, H, W, geom);
            hipStream_t s = ctx->stream;
            Scratch sc(ctx);
            // (a_rowidx / a_vals are checked once the count is known: an A without entries needs only its colptr)
            with_type(dtype, [&](auto tag) {
                using T = decltype(tag);
                const uint32_t *xr = to_device(sc, x_rows, nnz_x, space, s), *xc = to_device(sc, x_cols, nnz_x, space, s);
                const T *xv = to_device(sc, (const T *)x_vals, nnz_x, space, s);
                T *va = (T *)a_vals;
                *nnz_a = im2col_impl<T>(ctx, sc, N, C, g, nnz_x, xr, xc, xv, fill, a_colptr, a_rowidx, va);
            });
        });
        return OSP_OK;
    });
}

int osp_spgemm_conv2d(osp_context_t ctx_, osp_dtype_t dtype, uint64_t N, uint64_t C, uint64_t H, uint64_t W, uint64_t nnz_x,
                      const uint32_t *x_rows, const uint32_t *x_cols, const void *x_vals, uint64_t OC, uint64_t nnz_w,
                      const uint32_t *w_rows, const uint32_t *w_cols, const void *w_vals, osp_memspace_t space,
                      const osp_conv2d_geometry_t *geom, const osp_config_t *cfg_, osp_result_t *result) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !result) return fail(OSP_ERR_ARG, "null context or result pointer");
    if ((nnz_x && (!x_rows || !x_cols || !x_vals)) || (nnz_w && (!w_rows || !w_cols || !w_vals))) return fail(OSP_ERR_ARG, "null operand array");
    return guard([&] {
        check_dtype(dtype); check_space(space);
        if (!OC || OC > 0xffffffffull || nnz_x >= 0xffffffffull || nnz_w >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "OC must be >= 1; OC or nnz exceeds the u32 index type");
        const osp_config_t cfg = config_or_default(cfg_);
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            const ConvGeom g = conv_geometry(N, C, H, W, geom);
            spgemm_conv2d_impl<T>(ctx, res, N, C, g, nnz_x, x_rows, x_cols, (const T *)x_vals, OC, nnz_w, w_rows, w_cols, (const T *)w_vals,
                                  space, cfg);
        });
    });
}

int osp_csr_maxpool2d(osp_result_t in_, uint64_t N, uint64_t H, uint64_t W, uint32_t kh, uint32_t kw, uint32_t stride_h,
                      uint32_t stride_w, osp_result_t *out) {
    Result *in = (Result *)in_;
    if (!in || !out) return fail(OSP_ERR_ARG, "null argument");
    if (in->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    if (!N || !H || !W || !kh || !kw || !stride_h || !stride_w) return fail(OSP_ERR_ARG, "sizes, kernel and stride must be >= 1");
    if (H < kh || W < kw) return fail(OSP_ERR_ARG, "the pooling window is larger than the input: empty output");
    if (H >= 0xffffffffull || W >= 0xffffffffull || (unsigned __int128)N * H * W != in->info.M)
        return fail(OSP_ERR_ARG, "N*H*W must equal the rows of the input");
    return guard([&] {
        return new_result(in->ctx, in->dtype, out, [&](auto tag, Result *res) {   // (res->info: in's, variants included)
            maxpool_impl<decltype(tag)>(in->ctx, in, res, N, (uint32_t)H, (uint32_t)W, kh, kw, stride_h, stride_w);
        });
    });
}

// ---- what a plain stream reaches on this device (bench.py: roofline.peak_measured) ----
// 16 bytes per lane, one workgroup per 4 KB: the copy SURVEY.md 8d / BASELINE.md ask to be
// measured on the box beside the 8 TB/s of the data sheet (the reference prints its simulated DRAM rate,
// SimOuterSPACE.cpp:684-686).  rate = (bytes read + bytes written) / time.
int osp_stream_copy_probe(osp_context_t ctx_, uint64_t bytes, int reps, double *gbps) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !gbps) return fail(OSP_ERR_ARG, "null argument");
    if (bytes < 4096 || reps < 1 || reps > 1000) return fail(OSP_ERR_ARG, "bytes >= 4096, 1 <= reps <= 1000");
    return guard([&]() -> int {
        OSP_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        Scratch sc(ctx);
        const uint64_t n = bytes / sizeof(u32x4);
        u32x4 *src = sc.get<u32x4>(n), *dst = sc.get<u32x4>(n);
        OSP_HIP(hipMemsetAsync(src, 0x5a, n * sizeof(u32x4), s));
        if (n > 0xffffffffull * 256ull) return fail(OSP_ERR_ARG, "probe buffer too large");
        const unsigned grid = (unsigned)((n + 255) / 256);
        double best = 0;
        for (int nt = 0; nt < 2; nt++) {   // plain and non-temporal accesses: the better of the two is the measured roof
            for (int i = 0; i < 2; i++) {   // untimed: page tables, clocks
                if (nt) stream_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n); else stream_copy_kernel<false><<<grid, 256, 0, s>>>(src, dst, n);
            }
            EventPair ev;
            OSP_HIP(hipEventRecord(ev.a, s));
            for (int i = 0; i < reps; i++) {
                if (nt) stream_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n); else stream_copy_kernel<false><<<grid, 256, 0, s>>>(src, dst, n);
            }
            OSP_HIP(hipEventRecord(ev.b, s));
            OSP_HIP(hipStreamSynchronize(s));
            OSP_HIP(hipGetLastError());
            const double ms = ev.ms();
            if (ms > 0) best = std::max(best, 2.0 * (double)(n * sizeof(u32x4)) * reps / (ms * 1e-3) / 1e9);
        }
        *gbps = best;
        return OSP_OK;
    });
}

// ---- several GPUs of one node (osp_multi.h) ----
int osp_multi_context_create(const int *devices, int ndev, osp_multi_context_t *out) {
    if (!devices || !out) return fail(OSP_ERR_ARG, "null argument");
    if (ndev < 1 || ndev > OSP_MULTI_MAX_RANKS) return fail(OSP_ERR_ARG, "between 1 and %d ranks", OSP_MULTI_MAX_RANKS);
    return guard([&]() -> int {
        std::unique_ptr<MultiContext> mc(new MultiContext);
        for (int g = 0; g < ndev; g++) {
            osp_context_t c = nullptr;
            const int st = osp_context_create(devices[g], &c);
            if (st) return st;   // (the message is already set)
            mc->devices.push_back(devices[g]);
            mc->ctx.push_back((Context *)c);
            mc->copy.emplace_back((size_t)ndev, nullptr);
            mc->mctx.push_back(nullptr);
            osp_context_t c2 = nullptr;
            const int st2 = osp_context_create(devices[g], &c2);   // the merge of what arrives: a stream and a pool of its own
            if (st2) return st2;
            mc->mctx.back() = (Context *)c2;
            mc->ctx.back()->sibling = mc->mctx.back();
            mc->mctx.back()->sibling = mc->ctx.back();
            OSP_HIP(hipSetDevice(devices[g]));
            for (int h = 0; h < ndev; h++) {
                if (h == g) continue;
                OSP_HIP(hipStreamCreateWithFlags(&mc->copy[g][h], hipStreamNonBlocking));   // one stream per destination: one per link
            }
        }
        // direct copies between the GPUs where the hardware allows them (xGMI); without peer access a copy is staged
        // through the host by the runtime, which is slower but correct
        for (int g = 0; g < ndev; g++)
            for (int h = 0; h < ndev; h++) {
                if (devices[g] == devices[h]) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devices[g], devices[h]) == hipSuccess && can) {
                    (void)hipSetDevice(devices[g]);
                    (void)hipDeviceEnablePeerAccess(devices[h], 0);
                    (void)hipGetLastError();   // "already enabled" is fine
                }
            }
        *out = (osp_multi_context_t)mc.release();
        return OSP_OK;
    });
}
int osp_multi_context_destroy(osp_multi_context_t mc) {
    delete (MultiContext *)mc;
    return OSP_OK;
}

int osp_multi_operands_create(osp_multi_context_t mc_, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr,
                              const uint32_t *a_rowidx, const void *a_vals, const int64_t *b_rowptr, const uint32_t *b_colidx,
                              const void *b_vals, osp_multi_operands_t *out) {
    MultiContext *mc = (MultiContext *)mc_;
    if (!mc || !out || !a_colptr || !b_rowptr) return fail(OSP_ERR_ARG, "null argument");
    return guard([&]() -> int {
        check_dtype(dtype); check_dims(M, K, N);
        const int64_t nnz_a = a_colptr[K], nnz_b = b_rowptr[K];
        if (nnz_a < 0 || nnz_b < 0 || (uint64_t)nnz_a >= 0xffffffffull || (uint64_t)nnz_b >= 0xffffffffull)
            return fail(OSP_ERR_ARG, "operands with >= 2^32 non-zeros are not supported");
        if ((nnz_a && (!a_rowidx || !a_vals)) || (nnz_b && (!b_colidx || !b_vals))) return fail(OSP_ERR_ARG, "null operand array");
        for (uint64_t k = 0; k < K; k++)
            if (a_colptr[k + 1] < a_colptr[k] || b_rowptr[k + 1] < b_rowptr[k] || a_colptr[0] != 0 || b_rowptr[0] != 0)
                return fail(OSP_ERR_ARG, "pointer array is not a monotone 0..nnz sequence");
        std::unique_ptr<MultiOperands> ops(new MultiOperands);
        ops->mc = mc; ops->dtype = dtype; ops->M = M; ops->K = K; ops->N = N;
        with_type(dtype, [&](auto tag) {
            using T = decltype(tag);
            multi_upload<T>(mc, ops.get(), a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals);
        });
        *out = (osp_multi_operands_t)ops.release();
        return OSP_OK;
    });
}
int osp_multi_operands_destroy(osp_multi_operands_t ops) {
    delete (MultiOperands *)ops;
    return OSP_OK;
}

int osp_spgemm_multi(osp_multi_context_t mc_, osp_multi_operands_t ops_, const osp_config_t *cfg_, osp_multi_result_t *out) {
    MultiContext *mc = (MultiContext *)mc_;
    MultiOperands *ops = (MultiOperands *)ops_;
    if (!mc || !ops || !out) return fail(OSP_ERR_ARG, "null argument");
    if (ops->mc != mc) return fail(OSP_ERR_ARG, "operands belong to another multi-GPU context");
    return guard([&] {
        const osp_config_t cfg = config_or_default(cfg_);
        std::unique_ptr<MultiResult> res(new MultiResult);
        res->mc = mc;
        res->dtype = ops->dtype;
        if (cfg.validate) {
            // per slab, as the single-GPU entry point does: ordering, ranges, duplicates (233)
            for (size_t g = 0; g < mc->ctx.size(); g++) {
                Context *c = mc->ctx[g];
                OSP_HIP(hipSetDevice(c->device));
                const MultiOperands::Slab &sl = ops->slab[g];
                Scratch sc(c);
                uint32_t *flags = sc.get<uint32_t>(2);
                OSP_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), c->stream));
                if (sl.nnz_a) validate_idx_kernel<<<grid_for(sl.nnz_a, 256), 256, 0, c->stream>>>(sl.a_colptr, sl.a_rowidx, sl.K, sl.nnz_a, ops->M, flags);
                if (sl.nnz_b) validate_idx_kernel<<<grid_for(sl.nnz_b, 256), 256, 0, c->stream>>>(sl.b_rowptr, sl.b_colidx, sl.K, sl.nnz_b, ops->N, flags + 1);
                uint32_t fa = 0, fb = 0;
                { Gather gt(c->stream); gt.add(&fa, (const uint32_t *)flags); gt.add(&fb, (const uint32_t *)flags + 1); gt.wait(); }
                check_flags(fa, "A (CSC)");
                check_flags(fb, "B (CSR)");
            }
        }
        with_type(ops->dtype, [&](auto tag) { multi_product<decltype(tag)>(mc, ops, res.get(), cfg); });
        res->info.ms_upload = ops->ms_upload;
        *out = (osp_multi_result_t)res.release();
        return OSP_OK;
    });
}

int osp_spgemm_csc_csr_multi(const int *devices, int ndev, osp_dtype_t dtype, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr,
                             const uint32_t *a_rowidx, const void *a_vals, const int64_t *b_rowptr, const uint32_t *b_colidx,
                             const void *b_vals, const osp_config_t *cfg, osp_multi_context_t *mc_out, osp_multi_result_t *out) {
    if (!mc_out || !out) return fail(OSP_ERR_ARG, "null argument");
    osp_multi_context_t mc = nullptr;
    osp_multi_operands_t ops = nullptr;
    int st = osp_multi_context_create(devices, ndev, &mc);
    if (st) return st;
    st = osp_multi_operands_create(mc, dtype, M, K, N, a_colptr, a_rowidx, a_vals, b_rowptr, b_colidx, b_vals, &ops);
    if (st == OSP_OK) st = osp_spgemm_multi(mc, ops, cfg, out);
    if (ops) osp_multi_operands_destroy(ops);   // the result does not refer to the operands
    if (st) { osp_multi_context_destroy(mc); return st; }
    *mc_out = mc;   // the result's shards live in this context's pools: destroy the result first, then the context
    return OSP_OK;
}

int osp_multi_result_info(osp_multi_result_t r_, osp_multi_info_t *info) {
    MultiResult *r = (MultiResult *)r_;
    if (!r || !info) return fail(OSP_ERR_ARG, "null argument");
    *info = r->info;
    return OSP_OK;
}
int osp_multi_result_shard(osp_multi_result_t r_, int rank, uint64_t *row_begin, uint64_t *row_end, osp_result_t *shard) {
    MultiResult *r = (MultiResult *)r_;
    if (!r || rank < 0 || rank >= (int)r->shard.size()) return fail(OSP_ERR_ARG, "bad result or rank");
    if (row_begin) *row_begin = r->row_bounds[rank];
    if (row_end) *row_end = r->row_bounds[rank + 1];
    if (shard) *shard = (osp_result_t)r->shard[rank];
    return OSP_OK;
}
int osp_multi_result_copy_csr(osp_multi_result_t r_, int64_t *rowptr, uint32_t *colidx, void *vals) {
    MultiResult *r = (MultiResult *)r_;
    if (!r) return fail(OSP_ERR_ARG, "null result");
    const size_t vs = r->dtype == OSP_F32 ? 4 : 8;
    uint64_t base = 0;
    for (size_t g = 0; g < r->shard.size(); g++) {
        Result *sh = r->shard[g];
        const uint64_t r0 = r->row_bounds[g], nr = r->row_bounds[g + 1] - r0, nz = sh->info.nnz_c;
        const int st = osp_result_copy_csr((osp_result_t)sh, rowptr ? rowptr + r0 : nullptr, colidx ? colidx + base : nullptr,
                                           vals ? (char *)vals + base * vs : nullptr, OSP_HOST);
        if (st) return st;
        if (rowptr) for (uint64_t i = 0; i <= nr; i++) rowptr[r0 + i] += (int64_t)base;   // (entry nr is rewritten by the next shard)
        base += nz;
    }
    return OSP_OK;
}
int osp_multi_result_destroy(osp_multi_result_t r) {
    delete (MultiResult *)r;
    return OSP_OK;
}

int osp_result_info(osp_result_t r_, osp_result_info_t *info) {
    Result *r = (Result *)r_;
    if (!r || !info) return fail(OSP_ERR_ARG, "null argument");
    *info = r->info;
    return OSP_OK;
}

int osp_result_copy_csr(osp_result_t r_, int64_t *rowptr, uint32_t *colidx, void *vals, osp_memspace_t space) {
    Result *r = (Result *)r_;
    if (!r) return fail(OSP_ERR_ARG, "null result");
    if (r->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR: use osp_result_partials");
    return guard([&] {
        OSP_HIP(hipSetDevice(r->ctx->device));
        hipStream_t s = r->ctx->stream;
        const size_t vs = r->dtype == OSP_F32 ? 4 : 8;
        auto out = [&](void *dst, const void *src, size_t bytes) {
            if (space == OSP_HOST) copy_d2h(dst, src, bytes, s);
            else OSP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
        };
        if (rowptr) out(rowptr, r->rowptr, (r->info.M + 1) * sizeof(int64_t));
        if (colidx && r->info.nnz_c) out(colidx, r->colidx, r->info.nnz_c * sizeof(uint32_t));
        if (vals && r->info.nnz_c) out(vals, r->vals, r->info.nnz_c * vs);
        OSP_HIP(hipStreamSynchronize(s));
        return OSP_OK;
    });
}

int osp_result_device_ptrs(osp_result_t r_, const int64_t **rowptr, const uint32_t **colidx, const void **vals) {
    Result *r = (Result *)r_;
    if (!r) return fail(OSP_ERR_ARG, "null result");
    if (r->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR: use osp_result_partials");
    if (rowptr) *rowptr = r->rowptr;
    if (colidx) *colidx = r->colidx;
    if (vals) *vals = r->vals;
    return OSP_OK;
}

int osp_result_destroy(osp_result_t r_) {
    destroy_result((Result *)r_);
    return OSP_OK;
}

}  // extern "C"
