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
#include <optional>   // (osp_pipeline.h, included inside namespace osp below, cannot include it itself)
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
#include "../../include/outerspace_spgemm_mxm_masked.h"
#include "../../include/outerspace_spgemm_transpose.h"
#include "../../include/outerspace_spgemm_mxv.h"
#include "../../include/outerspace_spgemm_mxv_arg.h"
#include "../../include/outerspace_spgemm_mxd.h"
#include "../../include/outerspace_spgemm_sddmm.h"
#include "../../include/outerspace_spgemm_extract.h"
#include "../../include/outerspace_spgemm_build.h"
#include "../../include/outerspace_spgemm_assign.h"
#include "../../include/outerspace_spgemm_kron.h"
#include "../../include/outerspace_spgemm_select_k.h"
#include "../../include/outerspace_spgemm_scan.h"
#include "osp_internal.h"
#include "osp_paths.h"
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
#include "osp_mxv_arg.h"
#include "osp_mxd.h"
#include "osp_sddmm.h"
#include "osp_extract.h"
#include "osp_build.h"
#include "osp_assign.h"
#include "osp_kron.h"
#include "osp_select_k.h"
#include "osp_scan.h"

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

// ---- compressed operands on their way in --------------------------------------------------------------
// One compressed operand (CSC: A's columns; CSR: B's or a mask's rows): the caller's arrays, which the ingest replaces by
// their copies on the device.
struct CompressedIn {
    const int64_t *ptr; const uint32_t *idx; const void *val;
    size_t vbytes;             // bytes of a value (0: a pattern, no values)
    uint64_t nseg, bound;      // segments, and the dimension its indices lie in
    const char *what;          // its name in messages
    int64_t nnz = 0;
    const int64_t *ptr_host = nullptr;   // the caller's pointer array where it lives on the host
};
// Pointer arrays first: nnz comes from their last entries ...
template <size_t n>
static void operand_ptrs_in(Scratch &sc, hipStream_t s, osp_memspace_t space, CompressedIn (&ops)[n]) {
    for (CompressedIn &o : ops) {
        if (space == OSP_HOST) { o.ptr_host = o.ptr; o.nnz = o.ptr[o.nseg]; }
        o.ptr = to_device(sc, o.ptr, o.nseg + 1, space, s);
    }
}
// ... in one gathered read-back, to which `also` adds a word of the caller's; then the refusals, in the caller's words.
template <size_t n>
static void operand_nnz(hipStream_t s, osp_memspace_t space, CompressedIn (&ops)[n], const char *negative, const char *too_many,
                        uint64_t *also = nullptr, const uint64_t *also_dev = nullptr) {
    Gather g(s);
    if (space != OSP_HOST) for (CompressedIn &o : ops) g.add(&o.nnz, o.ptr + o.nseg);
    if (also) g.add(also, also_dev);
    g.wait();
    for (const CompressedIn &o : ops) if (o.nnz < 0) throw Error(OSP_ERR_ARG, negative);
    for (const CompressedIn &o : ops) if ((uint64_t)o.nnz >= 0xffffffffull) throw Error(OSP_ERR_ARG, too_many);
}
static void operand_entries_in(Scratch &sc, hipStream_t s, osp_memspace_t space, CompressedIn &o) {
    o.idx = to_device(sc, o.idx, (uint64_t)o.nnz, space, s);
    o.val = to_device(sc, (const char *)o.val, (uint64_t)o.nnz * o.vbytes, space, s);
}
// Operands on the device: pointers before indices (the index check walks the segments the pointer arrays describe), each
// pass ending in one gathered read-back of the operands' flags.  pointers = false: the index pass alone.
template <size_t n>
static void validate_operands(Scratch &sc, hipStream_t s, const CompressedIn (&ops)[n], bool pointers = true) {
    uint32_t *flags = sc.get<uint32_t>(n);
    OSP_HIP(hipMemsetAsync(flags, 0, n * sizeof(uint32_t), s));
    for (int pass = pointers ? 0 : 1; pass < 2; pass++) {
        for (size_t q = 0; q < n; q++) {
            const CompressedIn &o = ops[q];
            if (pass == 0) validate_ptr_kernel<<<grid_for(o.nseg + 1, 256), 256, 0, s>>>(o.ptr, o.nseg, o.nnz, flags + q);
            else if (o.nnz) validate_idx_kernel<<<grid_for(o.nnz, 256), 256, 0, s>>>(o.ptr, o.idx, o.nseg, o.nnz, o.bound, flags + q);
        }
        uint32_t f[n] = {};
        { Gather g(s); for (size_t q = 0; q < n; q++) g.add(&f[q], (const uint32_t *)flags + q); g.wait(); }
        for (size_t q = 0; q < n; q++) check_flags(f[q], ops[q].what);
    }
}

// ---- the stages of a product ---------------------------------------------------
// Stage 2: the k shard of the operands A and B (already on the device), then the row shard.
template <class T>
static Shard<T> shard_of(Context *ctx, Scratch &sc, PhaseTimer &tm, const osp_config_t &cfg, uint64_t M, const CompressedIn &A, const CompressedIn &B) {
    hipStream_t s = ctx->stream;
    const uint64_t K = A.nseg;
    Shard<T> sh{A.ptr, A.idx, (const T *)A.val, B.ptr, B.idx, (const T *)B.val, K, (uint64_t)B.nnz, cfg.k_begin, cfg.k_end ? cfg.k_end : K, 0, 0, 0, M};
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] spgemm M=%llu K=%llu N=%llu nnzA=%lld nnzB=%lld k=[%llu,%llu) %s operands\n", (unsigned long long)M,
                (unsigned long long)K, (unsigned long long)B.bound, (long long)A.nnz, (long long)B.nnz, (unsigned long long)sh.k0,
                (unsigned long long)sh.k1, A.ptr_host ? "host" : "device");
    if (sh.k0 > sh.k1 || sh.k1 > K) throw Error(OSP_ERR_ARG, "k range outside [0,K]");
    int64_t e1 = A.nnz;
    if (sh.k0 != 0 || sh.k1 != K) {
        if (A.ptr_host) { sh.e0 = A.ptr_host[sh.k0]; e1 = A.ptr_host[sh.k1]; }
        else { Gather g(s); g.add(&sh.e0, A.ptr + sh.k0); g.add(&e1, A.ptr + sh.k1); g.wait(); }
    }
    sh.nnz = (uint64_t)(e1 - sh.e0);
    if (cfg.row_shard_count > 1) {
        // The row shard: this rank's rows, and A without the rest -- same K columns, absolute row ids -- BEFORE the symbolic
        // phase (a rank then sorts 1/G of A's non-zeros instead of all of them; every rank derives the same bounds from the
        // replicated operands alone: no collective)
        const uint64_t nnz = sh.nnz;  // all of the k shard's non-zeros: the pre-pass sees every row
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
            const uint32_t stride = (sh.k1 - sh.k0) >= (1u << 16) ? 16u : 1u;
            const uint64_t nsample = (sh.k1 - sh.k0 + stride - 1) / stride;
            if (nnz) row_work_kernel<<<grid_for(nsample * kWave, 256), 256, 0, s>>>(sh.a_colptr, sh.a_rowidx, sh.b_rowptr, sh.k0, sh.k1, stride, work);
            device_exclusive_scan<LoadU64, uint64_t>(LoadU64{(const uint64_t *)work}, M, pre, tmp, s);
            device_exclusive_scan<RowCost, uint64_t>(RowCost{pre, (uint64_t)TileCap<T>::value, kSplitRowMax}, M, cost_pre, tmp, s);
            shard_bounds_kernel<<<grid_for(G + 1, 64), 64, 0, s>>>(cost_pre, pre, M, G, d_b, d_b + G + 1);
            std::vector<uint64_t> h_b(2ull * (G + 1));
            copy_d2h(h_b.data(), d_b, h_b.size() * sizeof(uint64_t), s);
            sh.r_lo = h_b[cfg.row_shard_index];
            sh.r_hi = h_b[cfg.row_shard_index + 1];
        }
        int64_t *colptr2 = sc.get<int64_t>(K + 1);
        {
            Scratch cs(ctx);
            uint32_t *keep_scan = cs.get<uint32_t>(nnz + 1);
            uint32_t *tmp = cs.get<uint32_t>(scan_scratch_entries(nnz + 1));
            const RowInRange keep{sh.a_rowidx + sh.e0, (uint32_t)sh.r_lo, sh.r_hi};
            device_exclusive_scan<RowInRange, uint32_t>(keep, nnz, keep_scan, tmp, s);
            const uint64_t nnz2 = d2h(keep_scan + nnz, s);
            uint32_t *rowidx2 = sc.get<uint32_t>(nnz2);
            T *vals2 = sc.get<T>(nnz2);
            restrict_colptr_kernel<<<grid_for(K + 1, 256), 256, 0, s>>>(sh.a_colptr, K, sh.e0, nnz, keep_scan, colptr2);
            if (nnz2) restrict_compact_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(keep, keep_scan, nnz, sh.a_vals + sh.e0, rowidx2, vals2);
            sh.a_colptr = colptr2; sh.a_rowidx = rowidx2; sh.a_vals = vals2;
            sh.e0 = 0;  // columns before k0 are empty now
            sh.nnz = nnz2;
        }
        tm.end(PH_SYM);
    }
    return sh;
}

// Stage 3's result: every row's offset into the staging, every chunk's (chunk = a non-zero of A times its row of B), and
// what the chosen formulations read of the chunk table.  Everything lives in the product's scratch.
template <class T> struct Symbolic {
    uint64_t *row_off = nullptr, *chunk_off = nullptr;
    uint64_t P = 0;                // partial products of the shard, or kPartialsOnDevice
    ChunkTable<T> ct{};            // row-wise variant
    uint32_t n_long_rows = 1;      // ... and how many rows it leaves to the multiply
    DirectSrc dsrc{};              // direct rows
    ShortRuns<T> srun{};           // gathered short rows
};

// Stage 3, the symbolic phase: chunk offsets in (row, k) order.  `paths`: which tables outlive it (ProductPaths{}: none,
// what a slab of the multi-GPU product asks for); read_p: the count of partial products comes to the host here.
template <class T>
static Symbolic<T> symbolic_phase(Context *ctx, Scratch &sc, uint64_t M, const Shard<T> &sh, const ProductPaths &paths, bool read_p) {
    hipStream_t s = ctx->stream;
    const uint64_t nnz = sh.nnz;
    Symbolic<T> sym;
    sym.row_off = sc.get<uint64_t>(M + 1);
    sym.chunk_off = sc.get<uint64_t>(nnz);
    if (nnz == 0) {
        OSP_HIP(hipMemsetAsync(sym.row_off, 0, (M + 1) * sizeof(uint64_t), s));
        return sym;
    }
    Scratch ss(ctx);
    Scratch &keep = paths.keep_table ? sc : ss;  // the chunk table outlives the symbolic phase
    const RowSort rs(ss, nnz, std::max(1, bits_for(M)));
    uint32_t *rows_sorted = (paths.gather_short ? keep : ss).template get<uint32_t>(nnz), *perm = keep.get<uint32_t>(nnz), *w_sorted = ss.get<uint32_t>(nnz);
    uint32_t *bs_sorted = paths.keep_table ? keep.get<uint32_t>(nnz) : nullptr;
    uint32_t *rowfirst = keep.get<uint32_t>(M + 1);
    uint64_t *offs_sorted = keep.get<uint64_t>(nnz + 1);
    uint64_t *scan_tmp = ss.get<uint64_t>(scan_scratch_entries(std::max<uint64_t>(nnz, M + 1)));
    // (row, k) order of A's non-zeros; the last sort pass also looks up each chunk's length
    T *av_sorted = paths.av_ride_along ? keep.get<T>(nnz) : nullptr;
    uint32_t *w = ss.get<uint32_t>(paths.av_ride_along ? 4 * nnz : paths.keep_table ? 2 * nnz : nnz);   // (kept table: (length, B row) pairs)
    uint32_t *bs = paths.keep_table ? w : nullptr;
    sym_chunk_len_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(sh.a_colptr, sh.b_rowptr, sh.k0, sh.k1, sh.e0, nnz, w, bs,
                                                            paths.av_ride_along ? reinterpret_cast<const uint32_t *>(sh.a_vals) : nullptr, (uint32_t)(sizeof(T) / 4));
    SymEpilogue sym_ep{w, bs, rows_sorted, perm, w_sorted, bs_sorted};
    if (paths.av_ride_along) { sym_ep.av_sorted = av_sorted; sym_ep.vwords = (uint32_t)(sizeof(T) / 4); }
    rs.sort(sh.a_rowidx + sh.e0, sym_ep);
    device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{w_sorted}, nnz, offs_sorted, scan_tmp, s);
    sym_row_offsets_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rows_sorted, offs_sorted, nnz, M, sym.row_off, rowfirst);
    const uint64_t rw_cap = (paths.rowwise || paths.gather_short) ? (uint64_t)TileCap<T>::value : 0ull;   // rows the multiply skips
    if (!paths.expand_rows) sym_scatter_offsets_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(perm, offs_sorted, rows_sorted, sym.row_off, rw_cap, nnz, sym.chunk_off);
    // (the product proper reads P together with the size of the result, merge_pipeline: one stream round trip less)
    sym.P = read_p ? d2h(offs_sorted + nnz, s) : kPartialsOnDevice;
    if (paths.direct) {
        DirectSrc &dsrc = sym.dsrc;
        dsrc = DirectSrc{rowfirst, offs_sorted, bs_sorted, perm, sh.b_colidx, sym.chunk_off, paths.direct_max};
        dsrc.b_rowptr = sh.b_rowptr; dsrc.K = sh.K; dsrc.nnz_b = sh.nnz_b; dsrc.keep = &sc;
        dsrc.gather = paths.gather_long;
        dsrc.expand_rows = paths.expand_rows;
        if (paths.expand_rows) { dsrc.chunk_off_ready = false; dsrc.rows_sorted = rows_sorted; dsrc.row_off = sym.row_off; dsrc.rw_cap = rw_cap; dsrc.nnz = nnz; }
        dsrc.a_vals = paths.av_ride_along ? (const void *)av_sorted : (const void *)(sh.a_vals + sh.e0); dsrc.av_in_order = paths.av_ride_along; dsrc.b_vals = sh.b_vals;
        if (dsrc.gather) {
            dsrc.gstat = (unsigned long long *)sc.get<uint64_t>(3);
            zero_async(s, {{dsrc.gstat, 3 * sizeof(uint64_t)}});
        }
    }
    if (paths.gather_short) {
        // the short rows' chunks as run descriptors, chunks without entries left out (once per product)
        const ShortRunFlag sf{offs_sorted};
        uint32_t *cidx = ss.get<uint32_t>(nnz + 1), *cidx_tmp = ss.get<uint32_t>(scan_scratch_entries(nnz + 1));
        device_exclusive_scan<ShortRunFlag, uint32_t>(sf, nnz, cidx, cidx_tmp, s);
        RunDesc<T> *runs0 = sc.get<RunDesc<T>>(nnz);   // (bound: every chunk; the count stays on the device)
        uint32_t *rowfirst0 = sc.get<uint32_t>(M + 1);
        short_runs_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(sf, cidx, nnz, bs_sorted, av_sorted, runs0);
        short_rowfirst_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rowfirst, cidx, M, rowfirst0);
        sym.srun = ShortRuns<T>{runs0, rowfirst0, sh.b_colidx, sh.b_vals};
    }
    if (paths.rowwise) {
        sym.ct = ChunkTable<T>{offs_sorted, bs_sorted, perm, rowfirst, sh.a_vals + sh.e0, sh.b_colidx, sh.b_vals, (uint32_t)rw_cap, 1u};
        uint32_t *flag_scan = ss.get<uint32_t>(M + 1);
        device_exclusive_scan<HeavyRowFlag, uint32_t>(HeavyRowFlag{sym.row_off, 0, (uint32_t)rw_cap}, M, flag_scan, (uint32_t *)scan_tmp, s);
        sym.n_long_rows = d2h(flag_scan + M, s);
    }
    return sym;
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

    // ---- 1. operands in ----
    CompressedIn ops[2] = {{a_colptr_in, a_rowidx_in, a_vals_in, sizeof(T), K, M, "A (CSC)"}, {b_rowptr_in, b_colidx_in, b_vals_in, sizeof(T), K, N, "B (CSR)"}};
    const CompressedIn &A = ops[0], &B = ops[1];
    // (with the pointer arrays comes the number of partial products of the whole product -- a sum over k of two differences:
    // what decides whether a product of few non-zeros still plans direct rows, osp_paths.h)
    uint64_t p_all = 0;
    operand_ptrs_in(sc, s, space, ops);
    unsigned long long *p_all_dev = (unsigned long long *)sc.get<uint64_t>(1);
    zero_async(s, {{p_all_dev, sizeof(uint64_t)}});
    // (few workgroups: every one ends in an atomic on ONE word, 11-13 ns apiece -- 3 579 of them were the 46 us this kernel
    // took on the web-Google shape)
    if (K) count_partials_kernel<<<(unsigned)std::min<uint64_t>(grid_for(K, 256), 256), 256, 0, s>>>(A.ptr, B.ptr, K, p_all_dev);
    operand_nnz(s, space, ops, "negative nnz in pointer array", "operands with >= 2^32 non-zeros are not supported", &p_all, (const uint64_t *)p_all_dev);
    for (CompressedIn &o : ops) operand_entries_in(sc, s, space, o);
    res->info.nnz_a = A.nnz;
    res->info.nnz_b = B.nnz;
    if (cfg.validate) validate_operands(sc, s, ops);

    // ---- 2. k shard and row shard, 3. symbolic phase ----
    const Shard<T> sh = shard_of<T>(ctx, sc, tm, cfg, M, A, B);
    const bool row_sharded = cfg.row_shard_count > 1;
    if (cfg.algorithm != OSP_ALGO_OUTER && cfg.algorithm != OSP_ALGO_ROWWISE) throw Error(OSP_ERR_ARG, "unknown algorithm");
    const ProductPaths paths = choose_paths(ctx->env, cfg.algorithm, sh.nnz, p_all, M, N, partials_only, PathLimits{kSplitRowMax, kDirectDenseMax});
    tm.begin(PH_SYM);
    const Symbolic<T> sym = symbolic_phase<T>(ctx, sc, M, sh, paths, partials_only || paths.rowwise || row_sharded);
    tm.end(PH_SYM);
    res->info.partials = sym.P;

    // ---- 4. producer ----
    OuterProducer<T> prod;
    prod.bind(ctx, res, sc, sh, sym.chunk_off, paths.gather_long);
    prod.nothing_staged = paths.rowwise && sym.n_long_rows == 0;
    prod.short_gathered = paths.gather_short;

    // ---- 5. partials-only exit or pipeline and statistics ----
    if (partials_only) {
        // osp_spgemm_partials: the multiply phase alone; offsets and records belong to the result
        if (row_sharded) throw Error(OSP_ERR_ARG, "partial products of a row shard are not supported");
        res->partials = true;
        res->rowptr = (int64_t *)ctx->alloc((M + 1) * sizeof(int64_t));
        OSP_HIP(hipMemcpyAsync(res->rowptr, sym.row_off, (M + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
        res->vals = ctx->alloc(std::max<uint64_t>(sym.P, 1) * sizeof(Part<T>));
        res->info.panels = 1;
        res->info.nnz_c = sym.P;
        res->info.row_begin = 0;
        res->info.row_end = M;
        tm.begin(PH_MUL);
        if (sym.P) prod.produce(PanelWork<T>{0, M, true, 0, sym.P, (Part<T> *)res->vals}, tm);
        tm.end(PH_MUL);
        finish_timing(res, ev, tm, s);
        return;
    }
    MergeRequest<T> rq{M, N, sym.row_off, sym.P, cfg.partial_capacity};
    rq.r_lo = sh.r_lo; rq.r_hi = sh.r_hi;
    rq.sink = sink;
    if (paths.rowwise) rq.ct = &sym.ct;
    if (paths.direct) rq.ds = &sym.dsrc;
    rq.short_runs = sym.srun;
    merge_pipeline<T>(ctx, res, prod, tm, rq);
    finish_timing(res, ev, tm, s);
    // what the gathered rows came to (after the product's timing: the read-back is not part of it)
    if (paths.gather_short) res->info.gathered_short_partials = res->info.partials - res->info.heavy_partials;
    if (sym.dsrc.gstat && res->info.direct_rows) {
        uint64_t gs[3] = {0, 0, 0};
        copy_d2h(gs, sym.dsrc.gstat, sizeof(gs), s);
        res->info.gathered_rows = gs[0]; res->info.gathered_partials = gs[1]; res->info.gathered_runs = gs[2];
    }
    if (ctx->env.verbose) {
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
    uint32_t *flags = ss.get<uint32_t>(1);
    OSP_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
    // stable LSD: by inner index first, then by segment
    const CooOrder o = coo_sort_two_keys(ss, nnz, inner, std::max(1, bits_for(ninner)), seg, std::max(1, bits_for(nseg)));
    ingest_finish_kernel<T><<<grid_for(nnz, 256), 256, 0, s>>>(o.outer_sorted, o.perm, inner, vals, nnz, nseg, ninner, idx, ov, flags);
    ingest_ptr_kernel<<<grid_for(nseg + 1, 256), 256, 0, s>>>(o.outer_sorted, nnz, nseg, ptr);
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
    CompressedIn pos[2] = {{(const int64_t *)a_pos, nullptr, nullptr, 0, K, M, "A (CSC)"}, {(const int64_t *)b_pos, nullptr, nullptr, 0, K, N, "B (CSR)"}};
    const char *const too_many = "operands with >= 2^32 non-zeros are not supported";
    operand_ptrs_in(sc, s, space, pos);
    operand_nnz(s, space, pos, too_many, too_many);
    const int64_t *ap = pos[0].ptr, *bp = pos[1].ptr;
    const int64_t nnz_a = pos[0].nnz, nnz_b = pos[1].nnz;
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
// a host array of device pointers, on the device
template <class P>
static const P *pointer_table(Scratch &sc, hipStream_t s, const std::vector<P> &h) {
    P *d = (P *)sc.get<void *>(h.size());
    copy_h2d(d, h.data(), h.size() * sizeof(void *), s);
    return d;
}
// through a device array of their row pointers (rp: the pointers themselves, on the host).
template <class Producer>
static void parts_symbolic(Context *ctx, Scratch &sc, PhaseTimer &tm, Result *res, const std::vector<const int64_t *> &rp, uint64_t M, Producer &prod) {
    hipStream_t s = ctx->stream;
    const int nparts = (int)rp.size();
    const int64_t *const *d_rp = pointer_table(sc, s, rp);
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

// One part of a parts merge on its way in: its row pointers (d: on the device) and its count of entries, refused when negative.
static uint64_t part_ptr_in(Scratch &sc, hipStream_t s, osp_memspace_t space, const int64_t *rowptr, uint64_t M, const char *negative, const int64_t *&d) {
    d = to_device(sc, rowptr, M + 1, space, s);
    const int64_t n = (space == OSP_HOST) ? rowptr[M] : d2h(d + M, s);
    if (n < 0) throw Error(OSP_ERR_ARG, negative);
    return (uint64_t)n;
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
        const uint64_t nnz = part_ptr_in(sc, s, space, rowptrs[p], M, "negative nnz in part", rp[p]);
        ci[p] = to_device(sc, colidxs[p], nnz, space, s);
        va[p] = to_device(sc, (const T *)valss[p], nnz, space, s);
        nnz_in += nnz;
    }
    res->info.nnz_a = nnz_in;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] merge_csr_parts M=%llu N=%llu parts=%d entries=%llu %s operands\n", (unsigned long long)M,
                (unsigned long long)N, nparts, (unsigned long long)nnz_in, space == OSP_HOST ? "host" : "device");
    PartsProducer<T> prod;
    prod.d_colidxs = pointer_table(sc, s, ci); prod.d_valss = pointer_table(sc, s, va);
    parts_symbolic(ctx, sc, tm, res, rp, M, prod);
    merge_pipeline<T>(ctx, res, prod, tm, MergeRequest<T>{M, N, prod.row_off, res->info.partials, cfg.partial_capacity});
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
    std::vector<uint64_t> count(nparts);
    for (int p = 0; p < nparts; p++) {
        count[p] = part_ptr_in(sc, s, space, rowptrs[p], M, "negative record count in part", rp[p]);
        rc[p] = to_device(sc, (const Part<T> *)records[p], count[p], space, s);
        res->info.nnz_a += count[p];
    }
    if (cfg.validate) {
        // offsets monotone from 0 to the record count, columns below N: what the split and dense paths index with
        uint32_t *flags = sc.get<uint32_t>(1);
        OSP_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
        for (int p = 0; p < nparts; p++) {
            const uint64_t n = count[p];
            validate_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(rp[p], M, n, flags);
            if (n) validate_record_cols_kernel<T><<<grid_for(n, 256), 256, 0, s>>>(rc[p], n, N, flags);
        }
        check_flags(d2h(flags, s), "record parts");
    }
    RecordPartsProducer<T> prod;
    prod.d_recs = pointer_table(sc, s, rc); prod.before = before;
    parts_symbolic(ctx, sc, tm, res, rp, M, prod);
    MergeRequest<T> rq{M, N, prod.row_off, res->info.partials, cfg.partial_capacity};
    rq.cuts = cuts;
    merge_pipeline<T>(ctx, res, prod, tm, rq);
    finish_timing(res, ev, tm, s);
}

// which of the two exact variants of the order-sensitive steps this context runs (visible in every result)
static void note_variants(const Context *ctx, Result *res) {
    res->info.rank_atomic = ctx->rank_atomic ? 1u : 0u;
    res->info.dense_atomic = ctx->dense_atomic[res->dtype == OSP_F64] ? 1u : 0u;
}

#include "osp_result_ops.h"

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
// Runs `body` on ctx's device, under one snapshot of the environment's settings (ctx->env).  When it throws, the stream is
// drained before the exception travels on: no buffer goes back to the pool while work queued on it may still use it.
template <class F>
static void on_device(Context *ctx, F &&body) {
    try {
        ctx->begin_call();
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
template <size_t N>
static void check_reserved(const uint32_t (&words)[N], const char *op) {
    for (uint32_t w : words)
        if (w) throw Error(OSP_ERR_ARG, std::string(op) + ": reserved words must be 0");
}
// What every entry point on CSR results refuses first, before guard: a null argument, then a result of osp_spgemm_partials.
// Returns OSP_OK when there is nothing to refuse.
static int refuse_operands(std::initializer_list<const Result *> in, bool others_given) {
    for (const Result *r : in)
        if (!r) others_given = false;
    if (!others_given) return fail(OSP_ERR_ARG, "null argument");
    for (const Result *r : in)
        if (r->partials) return fail(OSP_ERR_ARG, "a result of osp_spgemm_partials holds records, not a CSR");
    return OSP_OK;
}
// The frame of an entry point that makes a result from the CSR results `in` (others_given: its other required pointers are
// not null): check() throws the operation's own refusals, in its order; run(T{}, res, &st) fills a new result of the first
// operand's context and dtype.  *out and *stats are written when everything succeeded, and not otherwise.
template <class Stats, class Check, class Run>
static int csr_op(std::initializer_list<const Result *> in, bool others_given, osp_result_t *out, Stats *stats, Check &&check, Run &&run) {
    if (const int rc = refuse_operands(in, others_given && out)) return rc;
    return guard([&] {
        check();
        const Result *first = *in.begin();
        Stats st{};
        const int rc = new_result(first->ctx, first->dtype, out, [&](auto tag, Result *res) { run(tag, res, &st); });
        if (stats) *stats = st;
        return rc;
    });
}
// The same for an entry point that fills a vector of the caller's: run(T{}, &st).
template <class Stats, class Check, class Run>
static int csr_vector_op(const Result *in, bool others_given, Stats *stats, Check &&check, Run &&run) {
    if (const int rc = refuse_operands({in}, others_given)) return rc;
    return guard([&] {
        check();
        Stats st{};
        on_device(in->ctx, [&] { with_type(in->dtype, [&](auto tag) { run(tag, &st); }); });
        if (stats) *stats = st;
        return (int)OSP_OK;
    });
}

// what osp_csr_mxm and osp_csr_mxm_masked refuse of the semiring and the two operands, in this order
static void check_mxm(const Result *a, const Result *b, const osp_semiring_t *sr, const char *op) {
    const std::string o(op);
    if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX && sr->add != OSP_EWISE_FIRST)
        throw Error(OSP_ERR_ARG, o + ": add is not one of PLUS, MIN, MAX, FIRST");
    if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, o + ": mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
    check_reserved(sr->reserved, op);
    if (a->ctx != b->ctx) throw Error(OSP_ERR_ARG, o + ": the operands belong to different contexts");
    if (a->dtype != b->dtype) throw Error(OSP_ERR_ARG, o + ": the operands' dtypes differ");
    if (a->info.nnz_c >= 0xffffffffull || b->info.nnz_c >= 0xffffffffull)
        throw Error(OSP_ERR_ARG, o + ": operands with >= 2^32 - 1 non-zeros are not supported");
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
            const Settings &env = c->env;
            // OSP_RANK "ballot" | "atomic": debugging and tests/test_gpu_parity.py
            if (env.rank.is("ballot")) c->rank_atomic = false;
            else if (env.rank.is("atomic")) c->rank_atomic = true;
            if (c->rank_atomic) {
                Scratch sc(c);
                uint32_t *bad = sc.get<uint32_t>(1);
                OSP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
                rank_order_selftest_kernel<<<64, 256, 0, c->stream>>>(bad);
                if (d2h(bad, c->stream) != 0) {
                    c->rank_atomic = false;
                    if (env.verbose) fprintf(stderr, "[osp] LDS atomics do not return old values in lane order on this device: using ballot ranks\n");
                }
            }
            for (int wide = 0; wide < 2; wide++) {
                if (env.dense_add.is("ballot")) c->dense_atomic[wide] = false;
                else if (env.dense_add.is("atomic")) c->dense_atomic[wide] = true;
                if (!c->dense_atomic[wide]) continue;
                Scratch sc(c);
                uint32_t *bad = sc.get<uint32_t>(1);
                OSP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
                if (wide) fadd_order_selftest_kernel<double><<<64, 256, 0, c->stream>>>(bad);
                else fadd_order_selftest_kernel<float><<<64, 256, 0, c->stream>>>(bad);
                if (d2h(bad, c->stream) != 0) {
                    c->dense_atomic[wide] = false;
                    if (env.verbose)
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
        c->begin_call();
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
        // B's column view holds N + 1 offsets and A's row view M + 1, made by one thread per offset (ingest_ptr_kernel), and the
        // validation takes a thread per pointer of K + 1: beyond kThreadEachMax the launch is refused by the runtime (the call used
        // to fail there with a HIP error, after its first launches)
        if (std::max(std::max(M, K), N) + 1 > kThreadEachMax)
            throw Error(OSP_ERR_ARG, "masked product: M, K and N must be below 2^32 - 256 (the views take a thread per offset, N + 1 for B's)");
        return new_result(ctx, dtype, result, [&](auto tag, Result *res) {
            using T = decltype(tag);
            masked_impl<T>(ctx, res, M, K, N, a_colptr, a_rowidx, (const T *)a_vals, b_rowptr, b_colidx, (const T *)b_vals, m_rowptr,
                           m_colidx, space, cfg);
        });
    });
}

int osp_csr_inflate_prune(osp_result_t in_, const osp_mcl_step_t *step, int validate, osp_result_t *out, osp_mcl_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, step != nullptr, out, stats, [&] {
        if (!(step->power >= 1.0) || !(step->power < HUGE_VAL)) throw Error(OSP_ERR_ARG, "inflate_prune: power must be a finite number >= 1");
        if (!(step->threshold >= 0.0) || !(step->threshold < HUGE_VAL)) throw Error(OSP_ERR_ARG, "inflate_prune: threshold must be a finite number >= 0");
        check_reserved(step->reserved, "inflate_prune");
    }, [&](auto tag, Result *res, osp_mcl_stats_t *st) { inflate_prune_impl<decltype(tag)>(in->ctx, in, res, *step, validate, st); });
}

int osp_csr_apply_mask(osp_result_t in_, uint64_t M, uint64_t N, const int64_t *m_rowptr, const uint32_t *m_colidx, osp_memspace_t space,
                       int complement, int validate, osp_result_t *out, osp_apply_mask_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, m_rowptr != nullptr, out, stats, [&] {
        check_space(space);
        if (M != in->info.M || N != in->info.N) throw Error(OSP_ERR_ARG, "apply_mask: the mask's shape differs from the result's");
    }, [&](auto tag, Result *res, osp_apply_mask_stats_t *st) {
        apply_mask_impl<decltype(tag)>(in->ctx, in, res, m_rowptr, m_colidx, space, complement, validate, st);
    });
}

int osp_csr_select(osp_result_t in_, const osp_select_t *sel, osp_result_t *out, osp_select_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, sel != nullptr, out, stats, [&] {
        if (sel->op < OSP_SELECT_LT || sel->op > OSP_SELECT_OFFDIAG) throw Error(OSP_ERR_ARG, "select: op is not one of osp_select_op_t");
        check_reserved(sel->reserved, "select");
    }, [&](auto tag, Result *res, osp_select_stats_t *st) { select_impl<decltype(tag)>(in->ctx, in, res, *sel, st); });
}

int osp_csr_ewise(osp_result_t a_, osp_result_t b_, const osp_ewise_t *ew, osp_result_t *out, osp_ewise_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_;
    return csr_op({a, b}, ew != nullptr, out, stats, [&] {
        if (ew->mode != OSP_EWISE_UNION && ew->mode != OSP_EWISE_INTERSECT) throw Error(OSP_ERR_ARG, "ewise: mode is not one of osp_ewise_mode_t");
        if (ew->op < OSP_EWISE_PLUS || ew->op > OSP_EWISE_DIV) throw Error(OSP_ERR_ARG, "ewise: op is not one of osp_ewise_op_t");
        if (ew->mode == OSP_EWISE_UNION && (ew->op == OSP_EWISE_MINUS || ew->op == OSP_EWISE_DIV))
            throw Error(OSP_ERR_ARG, "ewise: MINUS and DIV are not defined for a union (an entry of b alone would be copied as it is)");
        check_reserved(ew->reserved, "ewise");
        if (a->ctx != b->ctx) throw Error(OSP_ERR_ARG, "ewise: the operands belong to different contexts");
        if (a->info.M != b->info.M || a->info.N != b->info.N) throw Error(OSP_ERR_ARG, "ewise: the operands' shapes differ");
        if (a->dtype != b->dtype) throw Error(OSP_ERR_ARG, "ewise: the operands' dtypes differ");
        if (a->info.nnz_c >= 0xffffffffull || b->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "ewise: operands with >= 2^32 - 1 non-zeros are not supported");
    }, [&](auto tag, Result *res, osp_ewise_stats_t *st) { ewise_impl<decltype(tag)>(a->ctx, a, b, res, *ew, st); });
}

int osp_csr_mxm(osp_result_t a_, osp_result_t b_, const osp_semiring_t *sr, osp_result_t *out, osp_mxm_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_;
    return csr_op({a, b}, sr != nullptr, out, stats, [&] {
        check_mxm(a, b, sr, "mxm");
        if (a->info.N != b->info.M) throw Error(OSP_ERR_DIM, "mxm: a's N differs from b's M");
    }, [&](auto tag, Result *res, osp_mxm_stats_t *st) { mxm_impl<decltype(tag)>(a->ctx, a, b, res, *sr, st); });
}

int osp_csr_mxm_masked(osp_result_t a_, osp_result_t b_, osp_result_t mask_, int complement, const osp_semiring_t *sr, osp_result_t *out,
                       osp_mxm_masked_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_, *mask = (Result *)mask_;
    return csr_op({a, b, mask}, sr != nullptr, out, stats, [&] {
        check_mxm(a, b, sr, "mxm_masked");
        if (mask->ctx != a->ctx) throw Error(OSP_ERR_ARG, "mxm_masked: the mask belongs to a different context");
        if (mask->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "mxm_masked: a mask with >= 2^32 - 1 entries is not supported");
        if (a->info.N != b->info.M) throw Error(OSP_ERR_DIM, "mxm_masked: a's N differs from b's M");
        if (mask->info.M != a->info.M || mask->info.N != b->info.N) throw Error(OSP_ERR_DIM, "mxm_masked: the mask's shape differs from (a's M, b's N)");
    }, [&](auto tag, Result *res, osp_mxm_masked_stats_t *st) {
        mxm_masked_impl<decltype(tag)>(a->ctx, a, b, mask, complement, res, *sr, st);
    });
}

int osp_csr_transpose(osp_result_t in_, const osp_transpose_t *tp, osp_result_t *out, osp_transpose_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, true, out, stats, [&] {
        if (tp) check_reserved(tp->reserved, "transpose");
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "transpose: an operand with >= 2^32 - 1 non-zeros is not supported");
        if (in->info.M > (1ull << 32)) throw Error(OSP_ERR_DIM, "transpose: a row index of in must fit a column of out");
        // out's N + 1 row pointers are written by one thread each (ingest_ptr_kernel)
        if (in->info.nnz_c && in->info.N + 1 > kThreadEachMax)
            throw Error(OSP_ERR_ARG, "transpose: a non-empty in must have N below 2^32 - 256 (out's N + 1 row pointers take one thread each)");
    }, [&](auto tag, Result *res, osp_transpose_stats_t *st) { transpose_impl<decltype(tag)>(in->ctx, in, res, st); });
}

int osp_csr_reduce(osp_result_t in_, int axis, int op, void *out_vec, osp_memspace_t space, osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_vector_op(in, out_vec != nullptr, stats, [&] {
        check_space(space);
        if (axis != OSP_AXIS_ROWS && axis != OSP_AXIS_COLS) throw Error(OSP_ERR_ARG, "reduce: axis is not one of osp_axis_t");
        if (op < OSP_REDUCE_PLUS || op > OSP_REDUCE_COUNT) throw Error(OSP_ERR_ARG, "reduce: op is not one of osp_reduce_op_t");
        if (axis == OSP_AXIS_COLS && in->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "reduce: the column axis does not support results with >= 2^32 - 1 non-zeros");
    }, [&](auto tag, osp_vector_stats_t *st) { reduce_impl<decltype(tag)>(in->ctx, in, axis, op, out_vec, space, st); });
}

int osp_csr_mxv(osp_result_t in_, const osp_semiring_t *sr, const void *x, void *y, osp_memspace_t space, osp_mxv_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_vector_op(in, sr && y, stats, [&] {
        check_space(space);
        if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX) throw Error(OSP_ERR_ARG, "mxv: add is not one of PLUS, MIN, MAX");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "mxv: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        check_reserved(sr->reserved, "mxv");
        if (!x && sr->mul != OSP_EWISE_FIRST) throw Error(OSP_ERR_ARG, "mxv: x may be null only when mul is FIRST");
    }, [&](auto tag, osp_mxv_stats_t *st) { mxv_impl<decltype(tag)>(in->ctx, in, *sr, x, y, space, st); });
}

int osp_csr_mxv_arg(osp_result_t in_, const osp_semiring_t *sr, const void *x, void *y, int64_t *arg, osp_memspace_t space,
                    osp_mxv_arg_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_vector_op(in, sr && arg, stats, [&] {
        check_space(space);
        if (sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX) throw Error(OSP_ERR_ARG, "mxv_arg: add is not one of MIN, MAX");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "mxv_arg: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        check_reserved(sr->reserved, "mxv_arg");
        if (!x && sr->mul != OSP_EWISE_FIRST) throw Error(OSP_ERR_ARG, "mxv_arg: x may be null only when mul is FIRST");
    }, [&](auto tag, osp_mxv_arg_stats_t *st) { mxv_arg_impl<decltype(tag)>(in->ctx, in, *sr, x, y, arg, space, st); });
}

int osp_csr_mxd(osp_result_t in_, const osp_semiring_t *sr, const void *x, uint64_t k, void *y, osp_memspace_t space, osp_mxd_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_vector_op(in, sr && y, stats, [&] {
        check_space(space);
        if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX) throw Error(OSP_ERR_ARG, "mxd: add is not one of PLUS, MIN, MAX");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "mxd: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        check_reserved(sr->reserved, "mxd");
        if (!x && sr->mul != OSP_EWISE_FIRST) throw Error(OSP_ERR_ARG, "mxd: x may be null only when mul is FIRST");
        if (k > kMxdMaxCols) throw Error(OSP_ERR_ARG, "mxd: k exceeds OSP_MXD_MAX_COLS");
    }, [&](auto tag, osp_mxd_stats_t *st) { mxd_impl<decltype(tag)>(in->ctx, in, *sr, x, k, y, space, st); });
}

int osp_csr_sddmm(osp_result_t in_, const osp_semiring_t *sr, int accum, const void *x, const void *y, uint64_t k, osp_memspace_t space,
                  osp_result_t *out, osp_sddmm_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, sr != nullptr, out, stats, [&] {
        check_space(space);
        if (sr->add != OSP_EWISE_PLUS && sr->add != OSP_EWISE_MIN && sr->add != OSP_EWISE_MAX) throw Error(OSP_ERR_ARG, "sddmm: add is not one of PLUS, MIN, MAX");
        if (sr->mul < OSP_EWISE_PLUS || sr->mul > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "sddmm: mul is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        check_reserved(sr->reserved, "sddmm");
        if (accum != OSP_VECTOR_NONE && (accum < OSP_EWISE_PLUS || accum > OSP_EWISE_DIV || accum == OSP_EWISE_FIRST))
            throw Error(OSP_ERR_ARG, "sddmm: accum is PLUS, TIMES, MINUS, DIV, MIN, MAX, SECOND or OSP_VECTOR_NONE");
        if (!x && sr->mul != OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "sddmm: x may be null only when mul is SECOND");
        if (!y && sr->mul != OSP_EWISE_FIRST) throw Error(OSP_ERR_ARG, "sddmm: y may be null only when mul is FIRST");
        if (k > kMxdMaxCols) throw Error(OSP_ERR_ARG, "sddmm: k exceeds OSP_MXD_MAX_COLS");
    }, [&](auto tag, Result *res, osp_sddmm_stats_t *st) { sddmm_impl<decltype(tag)>(in->ctx, in, res, *sr, accum, x, y, k, space, st); });
}

int osp_csr_apply_vectors(osp_result_t in_, const osp_vector_apply_t *ap, const void *x_rows, const void *y_cols, osp_memspace_t space,
                          osp_result_t *out, osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, ap != nullptr, out, stats, [&] {
        check_space(space);
        for (int32_t o : {ap->row_op, ap->col_op})
            if (o != OSP_VECTOR_NONE && (o < OSP_EWISE_PLUS || o > OSP_EWISE_DIV || o == OSP_EWISE_FIRST))
                throw Error(OSP_ERR_ARG, "apply_vectors: an op is PLUS, TIMES, MINUS, DIV, MIN, MAX, SECOND or OSP_VECTOR_NONE");
        if (ap->row_op == OSP_VECTOR_NONE && ap->col_op == OSP_VECTOR_NONE) throw Error(OSP_ERR_ARG, "apply_vectors: both sides are OSP_VECTOR_NONE");
        check_reserved(ap->reserved, "apply_vectors");
        if ((ap->row_op != OSP_VECTOR_NONE && !x_rows) || (ap->col_op != OSP_VECTOR_NONE && !y_cols))
            throw Error(OSP_ERR_ARG, "apply_vectors: a side with an op needs its vector");
    }, [&](auto tag, Result *res, osp_vector_stats_t *st) {
        apply_vectors_impl<decltype(tag)>(in->ctx, in, res, *ap, x_rows, y_cols, space, st);
    });
}

int osp_csr_select_vertices(osp_result_t in_, const uint8_t *keep_rows, const uint8_t *keep_cols, osp_memspace_t space, osp_result_t *out,
                            osp_vector_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, true, out, stats, [&] {
        check_space(space);
        if (!keep_rows && !keep_cols) throw Error(OSP_ERR_ARG, "select_vertices: keep_rows and keep_cols are both null");
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "select_vertices: results with >= 2^32 - 1 non-zeros are not supported");
    }, [&](auto tag, Result *res, osp_vector_stats_t *st) {
        select_vertices_impl<decltype(tag)>(in->ctx, in, res, keep_rows, keep_cols, space, st);
    });
}

int osp_csr_extract(osp_result_t in_, const osp_extract_t *ex, osp_result_t *out, osp_extract_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, ex != nullptr, out, stats, [&] {
        check_space(ex->space);
        check_reserved(ex->reserved, "extract");
        check_dims(ex->rows ? ex->n_rows : 0, 0, ex->cols ? ex->n_cols : 0);
        if (in->info.nnz_c >= 0xffffffffull) throw Error(OSP_ERR_ARG, "extract: results with >= 2^32 - 1 non-zeros are not supported");
    }, [&](auto tag, Result *res, osp_extract_stats_t *st) { extract_impl<decltype(tag)>(in->ctx, in, res, *ex, st); });
}

int osp_csr_assign(osp_result_t c_, osp_result_t a_, const osp_assign_t *as, osp_result_t *out, osp_assign_stats_t *stats) {
    Result *c = (Result *)c_, *a = (Result *)a_;
    return csr_op({c, a}, as != nullptr, out, stats, [&] {
        check_space(as->space);
        if (as->accum != OSP_ASSIGN_NO_ACCUM && (as->accum < OSP_EWISE_PLUS || as->accum > OSP_EWISE_SECOND))
            throw Error(OSP_ERR_ARG, "assign: accum is OSP_ASSIGN_NO_ACCUM or one of PLUS, TIMES, MIN, MAX, FIRST, SECOND");
        check_reserved(as->reserved, "assign");
        if (a->ctx != c->ctx) throw Error(OSP_ERR_ARG, "assign: the operands belong to different contexts");
        if (a->dtype != c->dtype) throw Error(OSP_ERR_ARG, "assign: the operands' dtypes differ");
        check_dims(as->rows ? as->n_rows : 0, 0, as->cols ? as->n_cols : 0);
        if (c->info.nnz_c >= 0xffffffffull || a->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "assign: operands with >= 2^32 - 1 non-zeros are not supported");
        if (a->info.M != (as->rows ? as->n_rows : c->info.M) || a->info.N != (as->cols ? as->n_cols : c->info.N))
            throw Error(OSP_ERR_DIM, "assign: a's shape is not (the number of rows, the number of columns) of the region");
    }, [&](auto tag, Result *res, osp_assign_stats_t *st) { assign_impl<decltype(tag)>(c->ctx, c, a, res, *as, st); });
}

int osp_csr_kron(osp_result_t a_, osp_result_t b_, const osp_kron_t *kr, osp_result_t *out, osp_kron_stats_t *stats) {
    Result *a = (Result *)a_, *b = (Result *)b_;
    static_assert(OSP_KRON_LAUNCHES == kKronLaunches, "the header states the kernels of the general path");
    return csr_op({a, b}, kr != nullptr, out, stats, [&] {
        if (kr->op < OSP_EWISE_PLUS || kr->op > OSP_EWISE_SECOND) throw Error(OSP_ERR_ARG, "kron: op is not one of TIMES, PLUS, MIN, MAX, FIRST, SECOND");
        check_reserved(kr->reserved, "kron");
        if (a->ctx != b->ctx) throw Error(OSP_ERR_ARG, "kron: the operands belong to different contexts");
        if (a->dtype != b->dtype) throw Error(OSP_ERR_ARG, "kron: the operands' dtypes differ");
        if (a->info.nnz_c >= 0xffffffffull || b->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_ARG, "kron: operands with >= 2^32 - 1 non-zeros are not supported");
        // (every dimension of a result is at most 2^32 - 1: the products fit 64 bits)
        check_dims(a->info.M * b->info.M, 0, a->info.N * b->info.N);
        if (a->info.nnz_c * b->info.nnz_c >= 0xffffffffull)
            throw Error(OSP_ERR_CAPACITY, "kron: the product would hold 2^32 - 1 entries or more");
    }, [&](auto tag, Result *res, osp_kron_stats_t *st) { kron_impl<decltype(tag)>(a->ctx, a, b, res, *kr, st); });
}

int osp_csr_select_k(osp_result_t in_, const osp_select_k_t *sk, osp_result_t *out, osp_select_k_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, sk != nullptr, out, stats, [&] {
        if (sk->order < OSP_SELECT_K_LARGEST || sk->order > OSP_SELECT_K_RANDOM) throw Error(OSP_ERR_ARG, "select_k: order is not one of osp_select_k_order_t");
        if (sk->k == 0) throw Error(OSP_ERR_ARG, "select_k: k must be at least 1");
        check_reserved(sk->reserved, "select_k");
    }, [&](auto tag, Result *res, osp_select_k_stats_t *st) { select_k_impl<decltype(tag)>(in->ctx, in, res, *sk, st); });
}

// (the kernels take a thread per block, per row and per entry chunk: see kThreadEachMax)
static void check_scan_size(const Result *in, const char *op) {
    if (in->info.nnz_c / kScanBlock + in->info.M > kThreadEachMax)
        throw Error(OSP_ERR_ARG, std::string(op) + ": nnz / 32 + M must be at most 2^32 - 256");
}

int osp_csr_scan(osp_result_t in_, const osp_scan_t *sc, osp_result_t *out, osp_scan_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_op({in}, sc != nullptr, out, stats, [&] {
        if (sc->op != OSP_REDUCE_PLUS && sc->op != OSP_REDUCE_MIN && sc->op != OSP_REDUCE_MAX) throw Error(OSP_ERR_ARG, "scan: op is not one of PLUS, MIN, MAX");
        check_reserved(sc->reserved, "scan");
        check_scan_size(in, "scan");
    }, [&](auto tag, Result *res, osp_scan_stats_t *st) { scan_impl<decltype(tag)>(in->ctx, in, res, *sc, st); });
}

int osp_csr_draw(osp_result_t in_, const osp_draw_t *dr, int64_t *cols, int64_t *pos, osp_memspace_t space, osp_draw_stats_t *stats) {
    Result *in = (Result *)in_;
    return csr_vector_op(in, dr && cols, stats, [&] {
        check_space(space);
        if (dr->draws == 0) throw Error(OSP_ERR_ARG, "draw: draws must be at least 1");
        if (in->info.M * (uint64_t)dr->draws > (1ull << 40)) throw Error(OSP_ERR_ARG, "draw: M * draws must be at most 2^40");
        if (dr->reserved0) throw Error(OSP_ERR_ARG, "draw: reserved words must be 0");
        check_reserved(dr->reserved, "draw");
        check_scan_size(in, "draw");
    }, [&](auto tag, osp_draw_stats_t *st) { draw_impl<decltype(tag)>(in->ctx, in, *dr, cols, pos, space, stats != nullptr, st); });
}

int osp_csr_build(osp_context_t ctx_, const osp_build_t *b, osp_result_t *out, osp_build_stats_t *stats) {
    Context *ctx = (Context *)ctx_;
    if (!ctx || !b || !out) return fail(OSP_ERR_ARG, "null argument");
    if (b->nnz && (!b->rows || !b->cols)) return fail(OSP_ERR_ARG, "build: null index list");
    return guard([&] {
        check_dtype(b->dtype); check_space(b->space);
        if (b->dup < 0 || b->dup >= DUP_OPS) throw Error(OSP_ERR_ARG, "build: dup must be an osp_dup_op_t");
        check_reserved(b->reserved, "build");
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
        ctx->begin_call();
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
        mc->begin_call();
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
        mc->begin_call();
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
                const CompressedIn slab[2] = {{sl.a_colptr, sl.a_rowidx, nullptr, 0, sl.K, ops->M, "A (CSC)", (int64_t)sl.nnz_a},
                                              {sl.b_rowptr, sl.b_colidx, nullptr, 0, sl.K, ops->N, "B (CSR)", (int64_t)sl.nnz_b}};
                validate_operands(sc, c->stream, slab, false);   // (the pointer arrays were checked on the host when the operands were made)
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
