// osp_result_ops.h -- the host side of the operations on results: what they share (the frame of a call, the two-pass and
// bit-compaction helpers) and every *_impl from bias_relu to draw, the conv stage and the masked product between them.  Part of
// the ONE translation unit osp_api.hip (included there, inside namespace osp, after osp_pipeline.h and the ingest); the kernels
// are in the headers the sections name.  DESIGN.md sections 8-20.
#pragma once

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
// a copy of `in`'s three arrays
template <class T>
static void copy_csr(const Result *in, Result *res, hipStream_t s) {
    const uint64_t M = in->info.M, nnz = in->info.nnz_c;
    alloc_rowptr(res, M);
    OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    alloc_entries<T>(res, nnz);
    OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    OSP_HIP(hipMemcpyAsync(res->vals, in->vals, nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
}
// the info of an M x N result that takes nothing over from an operand: every field the operation does not name stays 0
static void fresh_info(Result *res, uint64_t M, uint64_t K, uint64_t N) {
    res->info = osp_result_info_t{};
    res->info.dtype = res->dtype;
    res->info.M = M; res->info.K = K; res->info.N = N;
    res->info.row_begin = 0; res->info.row_end = M;
}
// The frame of such a call: its stream, its scratch and its clock, started here.
struct OpFrame {
    hipStream_t s;
    Scratch sc;
    EventPair ev;
    explicit OpFrame(Context *ctx) : s(ctx->stream), sc(ctx) { OSP_HIP(hipEventRecord(ev.a, s)); }
    // the end of the call's device work: waits for its stream; returns the call's time
    float stop() {
        OSP_HIP(hipEventRecord(ev.b, s));
        OSP_HIP(hipStreamSynchronize(s));
        OSP_HIP(hipGetLastError());
        return ev.ms();
    }
    // the end of a call that made `res`: stop(), then the result's size and the call's time
    void finish(Result *res, uint64_t nnz) {
        res->info.ms_total = stop();
        res->info.nnz_c = nnz;
    }
};
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
    fr.finish(res, nnz);
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
    fr.finish(res, nnz);
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
    const RowSort rs(ss, nnz, std::max(1, bits_for(nseg_major)));
    if (nseg_minor) csr_expand_rows_kernel<<<grid_for(nseg_minor * kWave, 256), 256, 0, s>>>(ptr, nseg_minor, minor);
    rs.sort(idx, MaskedViewEpilogue<T>{minor, vals, major, oidx, ovals});
    ingest_ptr_kernel<<<grid_for(nseg_major + 1, 256), 256, 0, s>>>(major, nnz, nseg_major, optr);
    OSP_HIP(hipStreamSynchronize(s));   // (ss goes back to the pool)
}

template <class T>
static void masked_impl(Context *ctx, Result *res, uint64_t M, uint64_t K, uint64_t N, const int64_t *a_colptr_in, const uint32_t *a_rowidx_in,
                        const T *a_vals_in, const int64_t *b_rowptr_in, const uint32_t *b_colidx_in, const T *b_vals_in,
                        const int64_t *m_rowptr_in, const uint32_t *m_colidx_in, osp_memspace_t space, const osp_config_t &cfg) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    EventPair ev_in, ev_k;
    fresh_info(res, M, K, N);   // (rank_atomic included)

    CompressedIn ops[3] = {{a_colptr_in, a_rowidx_in, a_vals_in, sizeof(T), K, M, "A (CSC)"}, {b_rowptr_in, b_colidx_in, b_vals_in, sizeof(T), K, N, "B (CSR)"},
                           {m_rowptr_in, m_colidx_in, nullptr, 0, M, N, "mask (CSR)"}};
    operand_ptrs_in(sc, s, space, ops);
    operand_nnz(s, space, ops, "negative nnz in pointer array", "operands or masks with >= 2^32 non-zeros are not supported");
    if (ops[2].nnz && !m_colidx_in) throw Error(OSP_ERR_ARG, "null mask column array with a non-empty mask");
    for (CompressedIn &o : ops) operand_entries_in(sc, s, space, o);
    const int64_t *a_colptr = ops[0].ptr, *b_rowptr = ops[1].ptr, *m_rowptr = ops[2].ptr;
    const uint32_t *a_rowidx = ops[0].idx, *b_colidx = ops[1].idx, *m_colidx = ops[2].idx;
    const T *a_vals = (const T *)ops[0].val, *b_vals = (const T *)ops[1].val;
    const int64_t nnz_a = ops[0].nnz, nnz_b = ops[1].nnz, nnz_m = ops[2].nnz;
    res->info.nnz_a = nnz_a;
    res->info.nnz_b = nnz_b;
    if (cfg.validate) validate_operands(sc, s, ops);

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
        const uint32_t heavy_min = (uint32_t)std::min<uint64_t>(ctx->env.masked_heavy_min.or_(kMaskedHeavyMin), 0xffffffffull);
        const int bucketed = ctx->env.masked_bucket.or_(1) ? 1 : 0;
        Scratch ss(ctx);
        uint32_t *key = ss.get<uint32_t>(nm), *order = ss.get<uint32_t>(nm);
        csr_expand_rows_kernel<<<grid_for(M * kWave, 256), 256, 0, s>>>(m_rowptr, M, m_row);
        masked_classify_kernel<<<grid_for(nm, 256), 256, 0, s>>>(m_row, m_colidx, arow_ptr, bcol_ptr, nm, heavy_min, bucketed, key, hit, count);
        uint32_t hc[kMaskedBuckets];
        copy_d2h(hc, count, sizeof(hc), s);
        const uint64_t n_empty = hc[kMaskedEmpty], n_heavy = hc[kMaskedHeavy], n_light = nm - n_empty - n_heavy;
        if (n_light || n_heavy) RowSort(ss, nm, 5).sort(key, MaskedOrderEpilogue{order});
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
    fr.finish(res, nnz_c);
    res->info.partials = P;
    res->info.ms_ingest = ev_in.ms();
    res->info.ms_multiply_kernel = ev_k.ms();
    res->info.multiply_launches = launches;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] masked M=%llu K=%llu N=%llu nnzA=%lld nnzB=%lld nnzM=%lld nnzC=%llu products=%llu launches=%u %.3f ms\n",
                (unsigned long long)M, (unsigned long long)K, (unsigned long long)N, (long long)nnz_a, (long long)nnz_b, (long long)nnz_m,
                (unsigned long long)nnz_c, (unsigned long long)P, launches, res->info.ms_total);
}

// ---- the step between two expansions of Markov clustering (osp_mcl.h) ----
template <class T>
static void inflate_prune_impl(Context *ctx, const Result *in, Result *res, const osp_mcl_step_t &step, int validate, osp_mcl_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    EventPair ev_k;
    const uint64_t M = in->info.M, nnz_in = in->info.nnz_c;
    const T *val = (const T *)in->vals;
    const T thr = (T)step.threshold, power = (T)step.power;
    const int mode = step.power == 1.0 ? MCL_POW_ONE : step.power == 2.0 ? MCL_POW_SQUARE : MCL_POW_GENERAL;
    const uint32_t long_min = (uint32_t)std::min<uint64_t>(ctx->env.mcl_long_min.or_(kMclLongMin), 0xffffffffull);
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
    fr.finish(res, nnz);
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
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] inflate_prune M=%llu nnz %llu -> %llu capped=%llu rescued=%llu long=%llu chaos=%.3e %.3f ms (select %.3f)\n",
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)nnz, (unsigned long long)capped, (unsigned long long)rescued,
                (unsigned long long)n_long, st->chaos, st->ms_total, st->ms_select_kernel);
}

// ---- the mask filter C<M> / C<¬M> of a CSR result (osp_apply_mask.h) ----
template <class T>
static void apply_mask_impl(Context *ctx, const Result *in, Result *res, const int64_t *m_rowptr_in, const uint32_t *m_colidx_in,
                            osp_memspace_t space, int complement, int validate, osp_apply_mask_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
        const CompressedIn mask[1] = {{m_rowptr, m_colidx, nullptr, 0, M, N, "mask (CSR)", nnz_m}};
        validate_operands(sc, s, mask);
        launches += nnz_m ? 3 : 2;   // (the flag's zeroing, the pointer check, the index check of a mask with entries)
    }

    res->info = in->info;
    Compacted c{0, 0};
    if (nnz_in && complement && have_nnz_m && nnz_m == 0) {
        // nothing is masked out: `in` itself
        c.nnz = nnz_in;
        copy_csr<T>(in, res, s);
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
    fr.finish(res, c.nnz);
    *st = osp_apply_mask_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_mask = (uint64_t)nnz_m;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (ctx->env.verbose)
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
    fr.finish(res, c.nnz);
    *st = osp_select_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = c.launches;
    if (ctx->env.verbose)
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
static void ewise_impl(Context *ctx, const Result *a, const Result *b, Result *res, const osp_ewise_t &ew, osp_ewise_stats_t *st) {
    typedef ValueBits<T> V;
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
    fr.finish(res, nnz_out);
    *st = osp_ewise_stats_t{};
    st->nnz_a = nnz_a;
    st->nnz_b = nnz_b;
    st->nnz_both = nnz_both;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] ewise %s op=%d M=%llu nnz %llu , %llu -> %llu (both %llu) launches=%u %.3f ms\n", uni ? "union" : "intersect", ew.op,
                (unsigned long long)M, (unsigned long long)nnz_a, (unsigned long long)nnz_b, (unsigned long long)nnz_out,
                (unsigned long long)nnz_both, launches, st->ms_total);
}

// ---- the product of two CSR results under a semiring, plain and at a mask (osp_mxm.h, DESIGN.md sections 15 and 27) ----
// (mask.rowptr is null for the plain product)
struct MxmOperands {
    const int64_t *a_rowptr; const uint32_t *a_col; const void *a_val;
    const int64_t *b_rowptr; const uint32_t *b_col; const void *b_val;
    const uint64_t *wscan;
    MxmMask mask;
};
template <class T, int ADD>
static void launch_mxm_short_add(const MxmOperands &op, hipStream_t s, uint64_t r0, uint64_t nrows, uint32_t cap, int mul, uint64_t p0, uint32_t *tcol,
                                 ValueBits<T> *tval, uint32_t *cnt) {
    typedef ValueBits<T> V;
    const auto kernel = op.mask.rowptr ? mxm_short_kernel<T, ADD, true> : mxm_short_kernel<T, ADD, false>;
    kernel<<<(unsigned)nrows, kWave, 0, s>>>(op.a_rowptr, op.a_col, (const V *)op.a_val, op.b_rowptr, op.b_col, (const V *)op.b_val, op.wscan, r0, cap,
                                             mul, p0, tcol, tval, cnt, op.mask);
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
                              uint64_t nprod, int colbits, uint64_t *key, uint32_t *pos, ValueBits<T> *pval, const uint32_t *kept_pos) {
    typedef ValueBits<T> V;
    if constexpr (MUL <= EW_SECOND) {
        if (mul == MUL) {
            const auto kernel = kept_pos ? mxm_expand_kernel<T, MUL, true> : mxm_expand_kernel<T, MUL, false>;
            kernel<<<grid_for(nprod, 256), 256, 0, s>>>(op.a_rowptr, op.a_col, (const V *)op.a_val, op.b_rowptr, op.b_col, (const V *)op.b_val, op.wscan,
                                                        long_rows, loff, nlong, nprod, colbits, key, pos, pval, kept_pos);
        } else launch_mxm_expand<T, MUL + 1>(mul, op, s, long_rows, loff, nlong, nprod, colbits, key, pos, pval, kept_pos);
    }
}
template <class T, int ADD>
static void launch_mxm_fold_add(const MxmOperands &op, hipStream_t s, const uint64_t *key, const ValueBits<T> *sorted_val, const uint64_t *headscan,
                                const uint64_t *head_pos, uint64_t nprod, const uint32_t *long_rows, const uint64_t *loff, int colbits, uint64_t p0,
                                uint32_t *tcol, ValueBits<T> *tval) {
    mxm_fold_kernel<T, ADD><<<grid_for(nprod, 256), 256, 0, s>>>(key, sorted_val, headscan, head_pos, nprod, op.a_rowptr, op.wscan, long_rows, loff,
                                                                 colbits, p0, tcol, tval);
}
// what a product counts, for the stats of either entry point
struct MxmCounts {
    uint64_t products = 0, kept = 0, nnz_out = 0, n_short = 0, n_long = 0;
    uint32_t nb = 0, launches = 0;
};
// The product of both entry points: `mask` null is osp_csr_mxm, launch for launch; with a mask only the products it admits
// (`complement`: rejects) are sorted and folded.  Fills res and its info and returns the counts; the caller writes its stats.
template <class T>
static MxmCounts mxm_run(Context *ctx, const Result *a, const Result *b, const Result *mask, int complement, Result *res,
                         const osp_semiring_t &sr) {
    typedef ValueBits<T> V;
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = a->info.M, K = a->info.N, N = b->info.N, nnz_a = a->info.nnz_c, nnz_b = b->info.nnz_c;
    fresh_info(res, M, K, N);
    res->info.nnz_a = nnz_a; res->info.nnz_b = nnz_b;
    uint64_t products = 0, nnz_out = 0, n_short = 0, n_long = 0, kept_long = 0;
    uint32_t nb = 0, launches = 0;
    // (an empty mask that is not complemented admits nothing: the symbolic phase still counts, no numeric kernel runs)
    const bool can_keep = !mask || complement || mask->info.nnz_c > 0;
    unsigned long long *kept_short = nullptr;

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
        const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ctx->env.mxm_short_cap.or_(kMxmShortMax), 1), kMxmShortMax);
        const uint64_t budget = std::min<uint64_t>(std::max<uint64_t>(ctx->env.mxm_batch.or_(kMxmBatchDefault), 1), 0xfffffffeull);
        if (mask) {
            kept_short = (unsigned long long *)sc.get<uint64_t>(1);
            zero_async(s, {{kept_short, sizeof(uint64_t)}});
        }
        const MxmOperands op{a->rowptr, a->colidx, a->vals, b->rowptr, b->colidx, b->vals, wscan,
                             mask ? MxmMask{mask->rowptr, mask->colidx, complement, kept_short} : MxmMask{nullptr, nullptr, 0, nullptr}};
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

        if (can_keep) alloc_rowptr(res, M); else empty_result<T>(res, M, s);
        uint32_t *cnt = sc.get<uint32_t>(M + 1);
        const int colbits = bits_for(N);
        struct BatchOut { uint32_t *col; V *val; uint64_t nnz; };
        std::vector<BatchOut> outs;
        for (uint32_t t = 0; t < nb && can_keep; t++) {
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
                    launches++;
                    // with a mask: a verdict per formed product, ONE scan and ONE read-back; from here on pl counts the KEPT
                    // products, koff holds the long rows' kept offsets, and loff stays what decodes a formed position
                    const uint64_t *koff = loff;
                    const uint32_t *kept_pos = nullptr;
                    if (mask) {
                        const uint64_t formed = pl, nwords = (formed + 63) / 64;
                        uint64_t *bits = sb.get<uint64_t>(nwords), *kpos = sb.get<uint64_t>(nwords + 1);
                        uint64_t *ktmp = sb.get<uint64_t>(scan_scratch_entries(nwords));
                        mxm_mask_flag_kernel<<<grid_for(formed, 256), 256, 0, s>>>(a->rowptr, a->colidx, b->rowptr, b->colidx, wscan, long_rows, loff,
                                                                                   (uint32_t)nl, formed, op.mask, bits);
                        launches += 1 + device_exclusive_scan<LoadPopc64, uint64_t>(LoadPopc64{bits}, nwords, kpos, ktmp, s);
                        pl = d2h((const uint64_t *)kpos + nwords, s);
                        uint32_t *list = sb.get<uint32_t>(std::max<uint64_t>(pl, 1));
                        uint64_t *kloff = sb.get<uint64_t>(nl + 1);
                        mxm_kept_list_kernel<<<grid_for(std::max(formed, nl + 1), 256), 256, 0, s>>>(bits, kpos, formed, loff, (uint32_t)nl, list, kloff);
                        launches++;
                        kept_long += pl;
                        koff = kloff;
                        kept_pos = list;
                    }
                    if (pl == 0) {   // (with a mask only) no long row of the batch keeps a product: no sort at all
                        mxm_long_empty_kernel<<<grid_for(nl, 256), 256, 0, s>>>(long_rows, (uint32_t)nl, cnt);
                        launches++;
                    } else {
                        SortedRuns runs(sb, pl);
                        V *pval = sb.get<V>(pl), *sorted_val = sb.get<V>(pl);
                        launch_mxm_expand<T>(sr.mul, op, s, long_rows, loff, (uint32_t)nl, pl, colbits, runs.keys[0], runs.poss[0], pval, kept_pos);
                        launches += 1 + runs.sort(colbits + bits_for(nl));
                        mxm_sorted_values_kernel<V><<<grid_for(pl, 256), 256, 0, s>>>(runs.poss[runs.cur], pval, pl, sorted_val);
                        launches += 1 + runs.heads();
                        const uint64_t *key = runs.keys[runs.cur], *headscan = runs.headscan, *head_pos = runs.head_pos();
                        if (sr.add == EW_PLUS) launch_mxm_fold_add<T, EW_PLUS>(op, s, key, sorted_val, headscan, head_pos, pl, long_rows, koff, colbits, p0, tcol, tval);
                        else if (sr.add == EW_MIN) launch_mxm_fold_add<T, EW_MIN>(op, s, key, sorted_val, headscan, head_pos, pl, long_rows, koff, colbits, p0, tcol, tval);
                        else if (sr.add == EW_MAX) launch_mxm_fold_add<T, EW_MAX>(op, s, key, sorted_val, headscan, head_pos, pl, long_rows, koff, colbits, p0, tcol, tval);
                        else launch_mxm_fold_add<T, EW_FIRST>(op, s, key, sorted_val, headscan, head_pos, pl, long_rows, koff, colbits, p0, tcol, tval);
                        mxm_long_counts_kernel<<<grid_for(nl, 256), 256, 0, s>>>(long_rows, koff, (uint32_t)nl, headscan, cnt);
                        launches += 2;   // (the list of run heads is counted by heads())
                    }
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
        if (nb > 1 && can_keep) {   // (nothing can be kept: empty_result made the whole result, no row has a count)
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
    MxmCounts c;
    if (kept_short) c.kept = (uint64_t)d2h((const uint64_t *)kept_short, s) + kept_long;
    fr.finish(res, nnz_out);
    res->info.partials = products;
    c.products = products;
    c.nnz_out = nnz_out;
    c.n_short = n_short;
    c.n_long = n_long;
    c.nb = nb;
    c.launches = launches;
    return c;
}
template <class T>
static void mxm_impl(Context *ctx, const Result *a, const Result *b, Result *res, const osp_semiring_t &sr, osp_mxm_stats_t *st) {
    const MxmCounts c = mxm_run<T>(ctx, a, b, nullptr, 0, res, sr);
    const uint64_t M = a->info.M, K = a->info.N, N = b->info.N, nnz_a = a->info.nnz_c, nnz_b = b->info.nnz_c;
    *st = osp_mxm_stats_t{};
    st->nnz_a = nnz_a;
    st->nnz_b = nnz_b;
    st->products = c.products;
    st->nnz_out = c.nnz_out;
    st->short_rows = c.n_short;
    st->long_rows = c.n_long;
    st->batches = c.nb;
    st->launches = c.launches;
    st->ms_total = res->info.ms_total;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] mxm add=%d mul=%d M=%llu K=%llu N=%llu nnz %llu , %llu -> %llu products=%llu short=%llu long=%llu batches=%u launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)K, (unsigned long long)N, (unsigned long long)nnz_a,
                (unsigned long long)nnz_b, (unsigned long long)c.nnz_out, (unsigned long long)c.products, (unsigned long long)c.n_short,
                (unsigned long long)c.n_long, c.nb, c.launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}
// the same product at a mask (include/outerspace_spgemm_mxm_masked.h)
template <class T>
static void mxm_masked_impl(Context *ctx, const Result *a, const Result *b, const Result *mask, int complement, Result *res,
                            const osp_semiring_t &sr, osp_mxm_masked_stats_t *st) {
    const MxmCounts c = mxm_run<T>(ctx, a, b, mask, complement ? 1 : 0, res, sr);
    *st = osp_mxm_masked_stats_t{};
    st->nnz_a = a->info.nnz_c;
    st->nnz_b = b->info.nnz_c;
    st->nnz_mask = mask->info.nnz_c;
    st->products = c.products;
    st->products_kept = c.kept;
    st->nnz_out = c.nnz_out;
    st->short_rows = c.n_short;
    st->long_rows = c.n_long;
    st->batches = c.nb;
    st->launches = c.launches;
    st->ms_total = res->info.ms_total;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] mxm_masked add=%d mul=%d complement=%d M=%llu K=%llu N=%llu nnz %llu , %llu mask %llu -> %llu products=%llu kept=%llu short=%llu long=%llu batches=%u launches=%u %.3f ms\n",
                sr.add, sr.mul, complement ? 1 : 0, (unsigned long long)a->info.M, (unsigned long long)a->info.N, (unsigned long long)b->info.N,
                (unsigned long long)st->nnz_a, (unsigned long long)st->nnz_b, (unsigned long long)st->nnz_mask, (unsigned long long)c.nnz_out,
                (unsigned long long)c.products, (unsigned long long)c.kept, (unsigned long long)c.n_short, (unsigned long long)c.n_long, c.nb,
                c.launches, st->ms_total);
}

// ---- the transpose of a CSR result (osp_transpose.h) ----
template <class T>
static void transpose_impl(Context *ctx, const Result *in, Result *res, osp_transpose_stats_t *st) {
    typedef ValueBits<T> V;
    typedef typename TrRecord<V>::type Rec;
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    fresh_info(res, N, in->info.K, M);
    res->info.nnz_a = nnz;
    uint32_t path = 0, passes = 0, launches = 0;
    if (nnz == 0) {
        empty_result<T>(res, N, s);
    } else if (M <= kTrMaskRows && !ctx->env.transpose_path.is("sort")) {
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
        passes = (uint32_t)rs_passes(nbits);
        const RowSort rs(sc, nnz, nbits);
        uint32_t *sorted_cols = sc.get<uint32_t>(nnz);
        if (ctx->env.transpose_gather.is("bisect")) {
            const TrEpilogue<V, false> epi{nullptr, in->rowptr, (const V *)in->vals, M, res->colidx, sorted_cols, (V *)res->vals};
            launches += rs.sort(in->colidx, epi);
        } else {
            Rec *rec = sc.get<Rec>(nnz);
            tr_pack_kernel<V><<<grid_for(nnz, (unsigned)kCompactChunk), kCompactThreads, 0, s>>>(in->rowptr, in->colidx, (const V *)in->vals, M, nnz, rec);
            launches++;
            const TrEpilogue<V, true> epi{rec, nullptr, nullptr, M, res->colidx, sorted_cols, (V *)res->vals};
            launches += rs.sort(in->colidx, epi);
        }
        ingest_ptr_kernel<<<grid_for(N + 1, 256), 256, 0, s>>>(sorted_cols, nnz, N, res->rowptr);
        launches++;
    }
    fr.finish(res, nnz);
    *st = osp_transpose_stats_t{};
    st->nnz = nnz;
    st->path = path;
    st->passes = passes;
    st->launches = launches;
    st->ms_total = res->info.ms_total;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] transpose M=%llu N=%llu nnz=%llu path=%u passes=%u launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, path, passes, launches, st->ms_total,
                (unsigned long long)ctx->malloc_calls);
}

// ---- a CSR result and dense vectors: reduce, apply, vertex select (osp_vector.h) ----
// The long segments of a level, listed and cut into blocks of kReduceBlock: segment long_segs[k] owns the blocks
// [blkptr[k], blkptr[k + 1]) and its result goes to next_map[k].  (blkptr, one stored accumulator per block) are the next
// level's segments.
struct LongCut {
    uint64_t n_long = 0, max_blocks = 0;
    const uint32_t *long_segs = nullptr, *next_map = nullptr;
    const int64_t *blkptr = nullptr;
};
// nent: an upper bound of the level's entries; map: where a segment's result goes (null: at its own number).  n_long is 0
// when no segment can be long (no kernel then) or none is; one read-back otherwise.  The one frame of reduce, mxv, mxv_arg
// and mxd.
static LongCut cut_long_segments(Scratch &sc, hipStream_t s, const int64_t *ptr, uint64_t nseg, uint64_t nent, const uint32_t *map, uint32_t &launches) {
    LongCut cut;
    if (nent <= kReduceBlock) return cut;
    unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(MCL_COUNTERS);
    zero_async(s, {{counters, MCL_COUNTERS * sizeof(uint64_t)}});
    uint32_t *long_segs = sc.get<uint32_t>(nent / ((uint64_t)kReduceBlock + 1) + 1);
    mcl_classify_kernel<<<grid_for(nseg, 256), 256, 0, s>>>(ptr, nseg, kReduceBlock, long_segs, counters);
    launches += 2;
    cut.n_long = d2h((const uint64_t *)counters + MCL_NLONG, s);
    if (!cut.n_long) return cut;
    // the long segments' blocks: sum ceil(m / block) <= nent / block + n_long, the exact number stays on the device
    cut.max_blocks = nent / kReduceBlock + cut.n_long;
    uint32_t *nblk = sc.get<uint32_t>(cut.n_long + 1), *next_map = sc.get<uint32_t>(cut.n_long);
    int64_t *blkptr = sc.get<int64_t>(cut.n_long + 1);
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(cut.n_long + 1));
    reduce_long_setup_kernel<<<grid_for(cut.n_long, 256), 256, 0, s>>>(ptr, long_segs, cut.n_long, map, nblk, next_map);
    launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{nblk}, cut.n_long, (uint64_t *)blkptr, tmp, s);
    cut.long_segs = long_segs;
    cut.next_map = next_map;
    cut.blkptr = blkptr;
    return cut;
}

// n stored accumulators from the pool: where a level's blocks kernel writes and the next level reads
template <class T>
static void get_stored(Scratch &sc, uint64_t n, Values<T> &v) {
    v.vals = sc.get<T>(n);
}
template <class T>
static void get_stored(Scratch &sc, uint64_t n, Pairs<T> &v) {
    v.vals = sc.get<T>(n);
    v.cols = sc.get<uint32_t>(n);
}

// R over every segment of (ptr, src) into out: the short segments by a wave each, the long ones block by block into a pool
// buffer whose segments (one per long segment) are the next level's input.  Acc is PlainAcc for reduce and mxv's upper
// levels, PairAcc for mxv_arg's.  long_segments: the first level's.
template <class Acc, class Sink>
static void reduce_segments(Scratch &sc, hipStream_t s, const int64_t *ptr, typename Acc::Stored src, uint64_t nseg, uint64_t nent, Sink out,
                            uint64_t &long_segments, uint32_t &launches, const uint32_t *map = nullptr) {
    for (int level = 0;; level++) {
        segments_short_kernel<Acc><<<grid_for(nseg, kReduceWaves), kReduceWaves * kWave, 0, s>>>(ptr, src, nseg, map, out);
        launches++;
        const LongCut cut = cut_long_segments(sc, s, ptr, nseg, nent, map, launches);
        if (level == 0) long_segments = cut.n_long;
        if (!cut.n_long) return;
        typename Acc::Stored partial;
        get_stored(sc, cut.max_blocks, partial);
        segments_blocks_kernel<Acc><<<grid_for(cut.max_blocks, kReduceWaves), kReduceWaves * kWave, 0, s>>>(ptr, src, cut.long_segs, cut.blkptr, cut.n_long,
                                                                                                            partial);
        launches++;
        ptr = cut.blkptr;
        src = partial;
        nseg = cut.n_long;
        nent = cut.max_blocks;
        map = cut.next_map;
    }
}

// the identity of the add `red` (RED_*; COUNT's, above them, is PLUS's) as a T
template <class T>
static T red_identity(int red) {
    const T inf = std::numeric_limits<T>::infinity();
    return red == RED_MIN ? inf : red == RED_MAX ? -inf : T(0);
}

// The last step of a dense result: the n values of the pool buffer `from` go to `to` in `space` -- or, when no kernel ran
// because every segment is empty, n times `fill`.  A null `to` is a vector the caller does not want.  The caller synchronises.
template <class T>
static void finish_dense(hipStream_t s, const T *from, void *to, uint64_t n, osp_memspace_t space, bool empty, T fill) {
    if (!n || !to) return;
    if (empty) {
        const std::vector<T> fills(n, fill);
        if (space == OSP_DEVICE) copy_h2d(to, fills.data(), n * sizeof(T), s);
        else memcpy(to, fills.data(), n * sizeof(T));
    } else if (space == OSP_DEVICE) {
#ifdef OSP_TEST_DENSE_SHORT   // (defined only to show that tests/result_chain.py notices an element of a caller's output that nothing wrote)
        n--;
#endif
        OSP_HIP(hipMemcpyAsync(to, from, n * sizeof(T), hipMemcpyDeviceToDevice, s));
    } else {
        copy_d2h(to, from, n * sizeof(T), s);
    }
}

template <class T>
static void reduce_impl(Context *ctx, const Result *in, int axis, int op, void *out_vec, osp_memspace_t space, osp_vector_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const uint64_t nout = axis == OSP_AXIS_ROWS ? M : N;
    uint64_t long_segments = 0;
    uint32_t launches = 0;
    // (the vector is formed in a pool buffer and copied out last: a call that fails leaves out_vec as it was)
    T *out = sc.get<T>(nout);
    if (nout && nnz) {
        const int64_t *ptr = in->rowptr;
        T *vals = (T *)in->vals;
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
        } else if (op == OSP_REDUCE_PLUS) {   // (vals is read only: Values is the sinks' type as well)
            reduce_segments<PlainAcc<RED_PLUS, T>>(sc, s, ptr, Values<T>{vals}, nout, nnz, Values<T>{out}, long_segments, launches);
        } else if (op == OSP_REDUCE_MIN) {
            reduce_segments<PlainAcc<RED_MIN, T>>(sc, s, ptr, Values<T>{vals}, nout, nnz, Values<T>{out}, long_segments, launches);
        } else {
            reduce_segments<PlainAcc<RED_MAX, T>>(sc, s, ptr, Values<T>{vals}, nout, nnz, Values<T>{out}, long_segments, launches);
        }
    }
    const float ms = fr.stop();
    finish_dense(s, out, out_vec, nout, space, !nnz, red_identity<T>(op));
    if (nout) OSP_HIP(hipStreamSynchronize(s));
    *st = osp_vector_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = nout;
    st->long_segments = long_segments;
    st->ms_total = ms;
    st->launches = launches;
    if (ctx->env.verbose)
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
static uint32_t mxv_group_log2(const Settings &env, uint64_t M, uint64_t nnz) {
    const uint64_t forced = env.mxv_group.or_(0);
    for (uint32_t lg = 2; lg <= 6; lg++)
        if (forced == (1ull << lg)) return lg;
    uint32_t lg = 2;
    while (lg < 6 && (M << lg) < nnz) lg++;
    return lg;
}

// R over every row of (rowptr, products) into out, for mxv (PlainAcc) and mxv_arg (PairAcc): the rows of at most
// kReduceBlock entries packed, the long ones block by block into stored accumulators, whose every further level is
// reduce_segments'.
template <class Acc, class Src, class Sink>
static void mxv_levels(Scratch &sc, hipStream_t s, const int64_t *rowptr, Src products, uint64_t M, uint64_t nnz, uint32_t lg, Sink out,
                       uint64_t &long_segments, uint32_t &launches) {
    const uint64_t waves = (M + (kWave >> lg) - 1) >> (6 - lg);
    segments_rows_kernel<Acc><<<grid_for(waves, kReduceWaves), kReduceWaves * kWave, 0, s>>>(rowptr, products, M, lg, out);
    launches++;
    const LongCut cut = cut_long_segments(sc, s, rowptr, M, nnz, nullptr, launches);
    long_segments = cut.n_long;
    if (!cut.n_long) return;
    typename Acc::Stored partial;
    get_stored(sc, cut.max_blocks, partial);
    segments_blocks_kernel<Acc><<<grid_for(cut.max_blocks, kReduceWaves), kReduceWaves * kWave, 0, s>>>(rowptr, products, cut.long_segs, cut.blkptr,
                                                                                                        cut.n_long, partial);
    launches++;
    uint64_t deeper = 0;
    reduce_segments<Acc>(sc, s, cut.blkptr, partial, cut.n_long, cut.max_blocks, out, deeper, launches, cut.next_map);
}

template <class T>
static void mxv_impl(Context *ctx, const Result *in, const osp_semiring_t &sr, const void *x_in, void *y_out, osp_memspace_t space,
                     osp_mxv_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const int add = sr.add == OSP_EWISE_PLUS ? RED_PLUS : sr.add == OSP_EWISE_MIN ? RED_MIN : RED_MAX;
    const uint32_t lg = mxv_group_log2(ctx->env, M, nnz);
    uint64_t long_segments = 0;
    uint32_t launches = 0;
    // (the vector is formed in a pool buffer and copied out last: x may be y, and a call that fails leaves y as it was)
    T *out = sc.get<T>(M);
    if (M && nnz) {
        const T *x = sr.mul == OSP_EWISE_FIRST ? nullptr : to_device(sc, (const T *)x_in, N, space, s);
        mxv_with_ops(add, sr.mul, [&](auto a, auto m) {
            constexpr int ADD = decltype(a)::value, MUL = decltype(m)::value;
            const Products<T, MUL> products{in->colidx, (const T *)in->vals, x};
            mxv_levels<PlainAcc<ADD, T>>(sc, s, in->rowptr, products, M, nnz, lg, Values<T>{out}, long_segments, launches);
        });
    }
    const float ms = fr.stop();
    finish_dense(s, out, y_out, M, space, !nnz, red_identity<T>(add));
    if (M) OSP_HIP(hipStreamSynchronize(s));
    *st = osp_mxv_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = M;
    st->long_segments = long_segments;
    st->group = 1u << lg;
    st->launches = launches;
    st->ms_total = ms;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] mxv add=%d mul=%d M=%llu N=%llu nnz=%llu group=%u long=%llu launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, 1u << lg, (unsigned long long)long_segments,
                launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- mxv with the winner's column (osp_mxv_arg.h) ----
template <class T>
static void mxv_arg_impl(Context *ctx, const Result *in, const osp_semiring_t &sr, const void *x_in, void *y_out, int64_t *arg_out,
                         osp_memspace_t space, osp_mxv_arg_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const int add = sr.add == OSP_EWISE_MIN ? RED_MIN : RED_MAX;
    const uint32_t lg = mxv_group_log2(ctx->env, M, nnz);
    uint64_t long_segments = 0, rows_without = M;
    uint32_t launches = 0;
    // (both vectors are formed in pool buffers and copied out last: x may be y, and a call that fails leaves y and arg as they
    // were.  y is formed whether the caller wants it or not: the kernels do not branch on it)
    T *out = sc.get<T>(M);
    int64_t *arg = sc.get<int64_t>(M);
    if (M && nnz) {
        const T *x = sr.mul == OSP_EWISE_FIRST ? nullptr : to_device(sc, (const T *)x_in, N, space, s);
        mxv_with_mul<RED_MIN>(sr.mul, [&](auto, auto m) {   // (the mul alone: the add is one of two)
            const Products<T, decltype(m)::value> products{in->colidx, (const T *)in->vals, x};
            const ArgSink<T> sink{out, arg};
            if (add == RED_MIN) mxv_levels<PairAcc<RED_MIN, T>>(sc, s, in->rowptr, products, M, nnz, lg, sink, long_segments, launches);
            else mxv_levels<PairAcc<RED_MAX, T>>(sc, s, in->rowptr, products, M, nnz, lg, sink, long_segments, launches);
        });
        // the stats' rows_without (few workgroups: each ends in one atomic on one word)
        unsigned long long *without = (unsigned long long *)sc.get<uint64_t>(1);
        zero_async(s, {{without, sizeof(uint64_t)}});
        arg_count_kernel<<<(unsigned)std::min<uint64_t>(grid_for(M, 256), 256), 256, 0, s>>>(arg, M, without);
        launches += 2;
        rows_without = d2h((const uint64_t *)without, s);
    }
    const float ms = fr.stop();
    finish_dense(s, out, y_out, M, space, !nnz, red_identity<T>(add));
    finish_dense(s, arg, arg_out, M, space, !nnz, (int64_t)-1);
    if (M) OSP_HIP(hipStreamSynchronize(s));
    *st = osp_mxv_arg_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = M;
    st->long_segments = long_segments;
    st->rows_without = rows_without;
    st->group = 1u << lg;
    st->launches = launches;
    st->ms_total = ms;
    if (ctx->env.verbose)
        fprintf(stderr,
                "[osp] mxv_arg add=%d mul=%d M=%llu N=%llu nnz=%llu group=%u long=%llu without=%llu launches=%u %.3f ms; pool misses so far: %llu "
                "hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, 1u << lg, (unsigned long long)long_segments,
                (unsigned long long)rows_without, launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- a CSR result times a dense matrix under a semiring (osp_mxd.h) ----
template <class T>
static void mxd_impl(Context *ctx, const Result *in, const osp_semiring_t &sr, const void *x_in, uint64_t k, void *y_out, osp_memspace_t space,
                     osp_mxd_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const int add = sr.add == OSP_EWISE_PLUS ? RED_PLUS : sr.add == OSP_EWISE_MIN ? RED_MIN : RED_MAX;
    uint32_t lgk = 0;   // log2 of the lanes a row gets: the power of two >= min(k, 64)
    while (lgk < 6 && (1ull << lgk) < k) lgk++;
    const uint32_t tiles = (uint32_t)((k + kWave - 1) / kWave);
    uint64_t long_segments = 0;
    uint32_t launches = 0;
    // (the matrix is formed in a pool buffer and copied out last: x may be y, and a call that fails leaves y as it was)
    T *out = sc.get<T>(M * k);
    if (M && k && nnz) {
        const T *x = sr.mul == OSP_EWISE_FIRST ? nullptr : to_device(sc, (const T *)x_in, N * k, space, s);
        const int64_t *rowptr = in->rowptr;
        const uint32_t *col = in->colidx;
        const T *vals = (const T *)in->vals;
        // a grid of (items << lgk) lanes by column tiles: 64 >> lgk items per wave
        const auto grid = [&](uint64_t items) { return dim3(grid_for((items + (kWave >> lgk) - 1) >> (6 - lgk), kReduceWaves), tiles); };
        mxv_with_ops(add, sr.mul, [&](auto a, auto m) {
            constexpr int ADD = decltype(a)::value, MUL = decltype(m)::value;
            mxd_rows_kernel<T, ADD, MUL><<<grid(M), kReduceWaves * kWave, 0, s>>>(rowptr, col, vals, x, M, k, lgk, out);
            launches++;
            // the long rows, listed and cut into blocks as mxv lists and cuts them
            const LongCut cut = cut_long_segments(sc, s, rowptr, M, nnz, nullptr, launches);
            long_segments = cut.n_long;
            if (!cut.n_long) return;
            T *partial = sc.get<T>(cut.max_blocks * k);
            mxd_blocks_kernel<T, ADD, MUL><<<grid(cut.max_blocks), kReduceWaves * kWave, 0, s>>>(rowptr, col, vals, x, cut.long_segs, cut.blkptr, cut.n_long, k,
                                                                                                 lgk, partial);
            mxd_upper_kernel<T, ADD><<<grid(cut.n_long), kReduceWaves * kWave, 0, s>>>(cut.long_segs, cut.blkptr, cut.n_long, partial, k, lgk, out);
            launches += 2;
        });
    }
    const float ms = fr.stop();
    finish_dense(s, out, y_out, M * k, space, !nnz, red_identity<T>(add));
    if (M && k) OSP_HIP(hipStreamSynchronize(s));
    *st = osp_mxd_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = M * k;
    st->cols = k;
    st->long_segments = long_segments;
    st->lanes_per_row = 1u << lgk;
    st->launches = launches;
    st->ms_total = ms;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] mxd add=%d mul=%d M=%llu N=%llu k=%llu nnz=%llu lanes=%u long=%llu launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, (unsigned long long)M, (unsigned long long)N, (unsigned long long)k, (unsigned long long)nnz, 1u << lgk,
                (unsigned long long)long_segments, launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- the sampled dense-dense product on a result's pattern (osp_sddmm.h) ----
template <class T>
static void sddmm_impl(Context *ctx, const Result *in, Result *res, const osp_semiring_t &sr, int accum, const void *x_in, const void *y_in, uint64_t k,
                       osp_memspace_t space, osp_sddmm_stats_t *st) {
    typedef ValueBits<T> V;
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const int add = sr.add == OSP_EWISE_PLUS ? RED_PLUS : sr.add == OSP_EWISE_MIN ? RED_MIN : RED_MAX;
    uint32_t lgk = 0;   // log2 of the lanes an entry gets: the power of two >= min(k, 64)
    while (lgk < 6 && (1ull << lgk) < k) lgk++;
    res->info = in->info;
    uint32_t launches = 0;
    if (M == 0 || nnz == 0) {
        empty_result<T>(res, M, s);
    } else {
        const T *x = sr.mul == OSP_EWISE_SECOND ? nullptr : to_device(sc, (const T *)x_in, M * k, space, s);
        // (x == y: one staging serves both)
        const T *y = sr.mul == OSP_EWISE_FIRST ? nullptr : y_in == x_in && x && M == N ? x : to_device(sc, (const T *)y_in, N * k, space, s);
        alloc_rowptr(res, M);
        OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        alloc_entries<T>(res, nnz);
        OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        mxv_with_ops(add, sr.mul, [&](auto a, auto m) {
            constexpr int ADD = decltype(a)::value, MUL = decltype(m)::value;
            // a wave per 64 entries
            sddmm_kernel<T, ADD, MUL><<<grid_for((nnz + kWave - 1) / kWave, kReduceWaves), kReduceWaves * kWave, 0, s>>>(
                in->rowptr, in->colidx, (const V *)in->vals, x, y, M, nnz, k, lgk, accum, (V *)res->vals);
            launches++;
        });
    }
    fr.finish(res, nnz);
    *st = osp_sddmm_stats_t{};
    st->nnz_in = st->nnz_out = nnz;
    st->cols = k;
    st->lanes_per_entry = 1u << lgk;
    st->launches = launches;
    st->ms_total = res->info.ms_total;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] sddmm add=%d mul=%d accum=%d M=%llu N=%llu k=%llu nnz=%llu lanes=%u launches=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                sr.add, sr.mul, accum, (unsigned long long)M, (unsigned long long)N, (unsigned long long)k, (unsigned long long)nnz, 1u << lgk, launches,
                st->ms_total, (unsigned long long)ctx->malloc_calls);
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
    fr.finish(res, nnz);
    *st = osp_vector_stats_t{};
    st->nnz_in = st->nnz_out = nnz;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] apply_vectors row_op=%d col_op=%d M=%llu nnz=%llu launches=%u %.3f ms\n", ap.row_op, ap.col_op, (unsigned long long)M,
                (unsigned long long)nnz, launches, st->ms_total);
}

template <class T>
static void select_vertices_impl(Context *ctx, const Result *in, Result *res, const uint8_t *keep_rows_in, const uint8_t *keep_cols_in,
                                 osp_memspace_t space, osp_vector_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz_in = in->info.nnz_c;
    res->info = in->info;
    const uint8_t *kr = keep_rows_in && nnz_in ? to_device(sc, keep_rows_in, M, space, s) : nullptr;
    const uint8_t *kc = keep_cols_in && nnz_in ? to_device(sc, keep_cols_in, N, space, s) : nullptr;
    const Compacted c = compact_by_bits<T>(sc, in, res, s, [&](unsigned nchunks, uint64_t *bits) {
        const auto flag = kr && kc ? vertex_flag_kernel<true, true> : kr ? vertex_flag_kernel<true, false> : vertex_flag_kernel<false, true>;
        flag<<<nchunks, kCompactThreads, 0, s>>>(in->rowptr, in->colidx, M, nnz_in, kr, kc, bits);
    });
    fr.finish(res, c.nnz);
    *st = osp_vector_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = c.nnz;
    st->ms_total = res->info.ms_total;
    st->launches = c.launches;
    if (ctx->env.verbose)
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
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
            if (ctx->env.extract_dense_map.is("1")) dense = sc.get<uint32_t>(N);
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
    fr.finish(res, nnz_out);
    *st = osp_extract_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_gathered = nnz_g;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (ctx->env.verbose)
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
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = b.M, N = b.N, nnz = b.nnz;
    const osp_memspace_t space = (osp_memspace_t)b.space;
    const int dup = b.dup;
    fresh_info(res, M, 0, N);
    note_variants(ctx, res);
    uint64_t nnz_out = 0, long_runs = 0;
    uint32_t launches = 0, readbacks = 0;
    if (nnz == 0 || M == 0 || N == 0) {
        empty_result<T>(res, M, s);
    } else {
        const bool has_vals = b.vals != nullptr && dup != DUP_COUNT;   // (COUNT reads no value: none is copied either)
        const bool folds = has_vals && (dup == DUP_PLUS || dup == DUP_MIN || dup == DUP_MAX);
        const uint32_t *rows = to_device(sc, b.rows, nnz, space, s), *cols = to_device(sc, b.cols, nnz, space, s);
        const V *vals = has_vals ? to_device(sc, (const V *)b.vals, nnz, space, s) : nullptr;
        int64_t *sptr = sc.get<int64_t>(M + 1);   // the sorted list's row pointer
        // (pool buffers are recycled, and OSP_POISON fills them: the error word and the counter are zeroed on every call)
        uint32_t *err = sc.get<uint32_t>(2);
        unsigned long long *n_long = sc.get<unsigned long long>(1);
        zero_async(s, {{err, sizeof(uint32_t)}, {n_long, sizeof(unsigned long long)}});
        launches++;
        // stable LSD: by column first, then by row
        const CooOrder o = coo_sort_two_keys(sc, nnz, cols, std::max(1, bits_for(N)), rows, std::max(1, bits_for(M)));
        const uint32_t *row_sorted = o.outer_sorted, *perm = o.perm;
        uint32_t *col_sorted = o.spare;
        ingest_gather_u32_kernel<<<grid_for(nnz, 256), 256, 0, s>>>(cols, perm, nnz, col_sorted);
        ingest_ptr_kernel<<<grid_for(M + 1, 256), 256, 0, s>>>(row_sorted, nnz, M, sptr);
        launches += o.launches + 2;
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
    fr.finish(res, nnz_out);
    *st = osp_build_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = nnz_out;
    st->long_runs = long_runs;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] build dup=%d vals=%d %llu x %llu nnz %llu -> %llu long_runs=%llu launches=%u readbacks=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                dup, b.vals != nullptr, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz, (unsigned long long)nnz_out,
                (unsigned long long)long_runs, launches, readbacks, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- out = c with the region (rows, cols) assigned from a (osp_assign.h) ----
template <class T, int OP = -1>
static void launch_assign_write_a(int op, unsigned grid, hipStream_t s, const Result *a, const Result *c, const AssignMaps &mp, const uint64_t *bits,
                                  const uint64_t *pos, Result *res) {
    typedef ValueBits<T> V;
    if constexpr (OP <= EW_SECOND) {
        if (op == OP)
            assign_write_a_kernel<T, OP><<<grid, kCompactThreads, 0, s>>>(a->rowptr, a->colidx, (const V *)a->vals, a->info.M, a->info.nnz_c, mp, c->rowptr,
                                                                         c->colidx, (const V *)c->vals, bits, pos, res->rowptr, res->colidx,
                                                                         (V *)res->vals);
        else launch_assign_write_a<T, OP + 1>(op, grid, s, a, c, mp, bits, pos, res);
    }
}

template <class T>
static void assign_impl(Context *ctx, const Result *c, const Result *a, Result *res, const osp_assign_t &as, osp_assign_stats_t *st) {
    typedef ValueBits<T> V;
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = c->info.M, N = c->info.N, nnz_c = c->info.nnz_c, nnz_a = a->info.nnz_c;
    const bool has_rows = as.rows != nullptr, has_cols = as.cols != nullptr, accum = as.accum != OSP_ASSIGN_NO_ACCUM;
    const uint64_t m = has_rows ? as.n_rows : M, n = has_cols ? as.n_cols : N;
    const osp_memspace_t space = (osp_memspace_t)as.space;
    res->info = c->info;
    uint64_t nnz_region = 0, nnz_both = 0, nnz_out = 0;
    uint32_t launches = 0, readbacks = 0;
    if (M == 0 || nnz_c + nnz_a == 0) {
        empty_result<T>(res, M, s);
    } else if (m == 0 || n == 0 || (accum && nnz_a == 0)) {
        copy_csr<T>(c, res, s);
        nnz_out = nnz_c;
    } else if (!has_rows && !has_cols && !accum) {
        copy_csr<T>(a, res, s);   // (the region is all of c)
        nnz_out = nnz_a;
    } else {
        // out's M row lengths are written by one thread each (assign_len_kernel)
        if (M > kThreadEachMax) throw Error(OSP_ERR_ARG, "assign: c must have at most 2^32 - 256 rows (out's row lengths take one thread each)");
        // (pool buffers are recycled, and OSP_POISON fills them: the error word, the counter and both maps are zeroed on every call)
        const uint64_t nwc = (N + 63) / 64, nwx = (nnz_c + 63) / 64;
        uint32_t *err = sc.get<uint32_t>(1);
        unsigned long long *other = sc.get<unsigned long long>(1);
        uint32_t *rmap = has_rows ? sc.get<uint32_t>(M) : nullptr;
        uint64_t *colbits = has_cols ? sc.get<uint64_t>(nwc) : nullptr;
        uint32_t *cpos = has_cols ? sc.get<uint32_t>(nwc + 1) : nullptr;   // (ranks of columns: below n <= 2^32 - 1)
        zero_async(s, {{err, sizeof(uint32_t)}, {other, sizeof(unsigned long long)}, {rmap, has_rows ? M * sizeof(uint32_t) : 0},
                       {colbits, has_cols ? nwc * sizeof(uint64_t) : 0}});
        launches++;
        AssignMaps mp{};
        if (has_rows) {
            mp.rows = to_device(sc, as.rows, m, space, s);
            mp.rmap = rmap;
            assign_rowmap_kernel<<<grid_for(m, 256), 256, 0, s>>>(mp.rows, m, M, rmap, err);
            launches++;
        }
        if (has_cols) {
            mp.cols = to_device(sc, as.cols, n, space, s);
            mp.colbits = colbits;
            mp.cpos = cpos;
            uint32_t *tmp = sc.get<uint32_t>(scan_scratch_entries(nwc));
            extract_colmap_kernel<<<grid_for(n, 256), 256, 0, s>>>(mp.cols, n, N, (unsigned long long *)colbits, nullptr, err);
            launches += 1 + device_exclusive_scan<LoadPopc64, uint32_t>(LoadPopc64{colbits}, nwc, cpos, tmp, s);
        }
        // The flag pass reads the maps, which hold only what a good index wrote, and writes scratch alone: the error word
        // travels with its count in the call's one read-back, and nothing of out is written before the lists are known good.
        uint32_t bad = 0;
        uint64_t n_other = 0;
        const auto more = [&](Gather &ga) {
            ga.add(&bad, (const uint32_t *)err);
            ga.add(&n_other, (const uint64_t *)other);
        };
        BitScan x{nullptr, nullptr, 0, 0};
        if (nnz_c) {
            x = flag_and_scan(sc, nnz_c, s, [&](unsigned grid, uint64_t *bits) {
                const auto flag = accum ? assign_flag_kernel<true> : assign_flag_kernel<false>;
                flag<<<grid, kCompactThreads, 0, s>>>(c->rowptr, c->colidx, M, nnz_c, mp, a->rowptr, a->colidx, bits, other);
            }, more);
        } else {   // an embedding: no bit, and a scan of one zero word in the arrays' place
            x.bits = sc.get<uint64_t>(nwx + 1);
            x.pos = sc.get<uint64_t>(nwx + 2);
            zero_async(s, {{x.bits, (nwx + 1) * sizeof(uint64_t)}, {x.pos, (nwx + 2) * sizeof(uint64_t)}});
            x.launches = 1;
            Gather ga(s);
            more(ga);
            ga.wait();
        }
        readbacks++;
        launches += x.launches;
        if (bad & kAssignBadRow) throw Error(OSP_ERR_ARG, "assign: a row index is not below the rows of c");
        if (bad & kAssignRepeatedRow) throw Error(OSP_ERR_ARG, "assign: a row index is repeated");
        if (bad & kAssignBadCol) throw Error(OSP_ERR_ARG, "assign: the columns are not strictly ascending and below the columns of c");
        nnz_region = accum ? n_other : x.count;
        nnz_both = accum ? x.count : n_other;
        nnz_out = nnz_c + nnz_a - x.count;
        alloc_rowptr(res, M);
        alloc_entries<T>(res, nnz_out);
        uint32_t *len = sc.get<uint32_t>(M);
        uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(M));
        assign_len_kernel<<<grid_for(M, 256), 256, 0, s>>>(c->rowptr, M, mp, a->rowptr, x.bits, x.pos, len);
        launches += 1 + device_exclusive_scan<LoadU32As64, uint64_t>(LoadU32As64{len}, M, (uint64_t *)res->rowptr, tmp, s);
        if (x.count < nnz_c) {   // (else c has no entry left of its own)
            assign_write_c_kernel<V><<<grid_for(nnz_c, (unsigned)kCompactChunk), kCompactThreads, 0, s>>>(
                c->rowptr, c->colidx, (const V *)c->vals, M, nnz_c, mp, a->rowptr, a->colidx, x.bits, x.pos, res->rowptr, res->colidx, (V *)res->vals);
            launches++;
        }
        if (nnz_a) {
            launch_assign_write_a<T>(as.accum, grid_for(nnz_a, (unsigned)kCompactChunk), s, a, c, mp, x.bits, x.pos, res);
            launches++;
        }
    }
    fr.finish(res, nnz_out);
    *st = osp_assign_stats_t{};
    st->nnz_c = nnz_c;
    st->nnz_a = nnz_a;
    st->nnz_region = nnz_region;
    st->nnz_both = nnz_both;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] assign rows=%d cols=%d accum=%d %llu x %llu into %llu x %llu nnz %llu , %llu -> %llu (region %llu, both %llu) launches=%u readbacks=%u %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                has_rows, has_cols, as.accum, (unsigned long long)m, (unsigned long long)n, (unsigned long long)M, (unsigned long long)N,
                (unsigned long long)nnz_c, (unsigned long long)nnz_a, (unsigned long long)nnz_out, (unsigned long long)nnz_region,
                (unsigned long long)nnz_both, launches, readbacks, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- out = a (x) b, the Kronecker product (osp_kron.h) ----
template <class T, int OP = 0>
static void launch_kron_entries(int op, unsigned grid, hipStream_t s, const Result *a, const Result *b, uint64_t nnz_out, Result *res) {
    typedef ValueBits<T> V;
    if constexpr (OP <= EW_SECOND) {
        if (op == OP)
            kron_entries_kernel<T, OP><<<grid, kKronThreads, 0, s>>>(a->rowptr, a->colidx, (const V *)a->vals, (uint32_t)a->info.M, b->rowptr, b->colidx,
                                                                     (const V *)b->vals, (uint32_t)b->info.M, (uint32_t)b->info.N, b->info.nnz_c, nnz_out,
                                                                     res->colidx, (V *)res->vals);
        else launch_kron_entries<T, OP + 1>(op, grid, s, a, b, nnz_out, res);
    }
}

// (the entry point has checked the shape of out and that nnz_a nnz_b is below 2^32 - 1)
template <class T>
static void kron_impl(Context *ctx, const Result *a, const Result *b, Result *res, const osp_kron_t &kr, osp_kron_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    const uint64_t M = a->info.M * b->info.M, N = a->info.N * b->info.N, nnz_a = a->info.nnz_c, nnz_b = b->info.nnz_c;
    fresh_info(res, M, 0, N);
    res->info.nnz_a = nnz_a; res->info.nnz_b = nnz_b;
    uint64_t nnz_out = 0;
    uint32_t launches = 0;
    if (M == 0 || nnz_a == 0 || nnz_b == 0) {
        empty_result<T>(res, M, s);
    } else {
        // the host knows the size of out: nothing is read back, and out's three arrays are the call's only allocations
        nnz_out = nnz_a * nnz_b;
        alloc_rowptr(res, M);
        alloc_entries<T>(res, nnz_out);
        kron_rowptr_kernel<<<std::min(grid_for(M + 1, 256), kKronRowBlocks), 256, 0, s>>>(a->rowptr, b->rowptr, M, (uint32_t)b->info.M, nnz_b, res->rowptr);
        launch_kron_entries<T>(kr.op, grid_for(nnz_out, (unsigned)kKronChunk), s, a, b, nnz_out, res);
        launches = kKronLaunches;
    }
    fr.finish(res, nnz_out);
    res->info.partials = nnz_out;
    *st = osp_kron_stats_t{};
    st->nnz_a = nnz_a;
    st->nnz_b = nnz_b;
    st->nnz_out = nnz_out;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = 0;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] kron op=%d (%llu x %llu, nnz %llu) (x) (%llu x %llu, nnz %llu) -> %llu x %llu, nnz %llu launches=%u readbacks=0 %.3f ms; pool misses so far: %llu hipMalloc calls\n",
                kr.op, (unsigned long long)a->info.M, (unsigned long long)a->info.N, (unsigned long long)nnz_a, (unsigned long long)b->info.M,
                (unsigned long long)b->info.N, (unsigned long long)nnz_b, (unsigned long long)M, (unsigned long long)N, (unsigned long long)nnz_out,
                launches, st->ms_total, (unsigned long long)ctx->malloc_calls);
}

// ---- the row-wise k-select of a CSR result (osp_select_k.h) ----
template <class F, int ORDER = 0>
static void with_select_k_order(int order, F &&body) {
    if constexpr (ORDER < SELK_ORDERS) {
        if (order == ORDER) body(std::integral_constant<int, ORDER>{});
        else with_select_k_order<F, ORDER + 1>(order, std::forward<F>(body));
    }
}

template <class T>
static void select_k_impl(Context *ctx, const Result *in, Result *res, const osp_select_k_t &sk, osp_select_k_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, N = in->info.N, nnz_in = in->info.nnz_c;
    const uint32_t k = sk.k;
    res->info = in->info;
    uint64_t nnz = nnz_in, n_wave = 0, n_long = 0;
    uint32_t launches = 0, readbacks = 0;
    if (nnz_in == 0) {
        empty_result<T>(res, M, s);
    } else if (k >= std::min(N, nnz_in)) {
        copy_csr<T>(in, res, s);   // no row can hold more than k entries: `in` itself, and nothing to ask the device
    } else {
        with_select_k_order(sk.order, [&](auto order_tag) {
            constexpr int ORDER = decltype(order_tag)::value;
            typedef typename SelectKKey<T, ORDER>::type K;
            const uint64_t seed = select_k_mix(sk.seed + 0x9E3779B97F4A7C15ull);
            const T *val = (const T *)in->vals;
            // ---- classes: at most nnz / (k + 1) rows are longer than k ----
            unsigned long long *counters = (unsigned long long *)sc.get<uint64_t>(SELK_COUNTERS);
            uint32_t *wave_rows = sc.get<uint32_t>(nnz_in / ((uint64_t)k + 1) + 1);
            uint32_t *long_rows = sc.get<uint32_t>(nnz_in / ((uint64_t)std::max(k, kSelectKLongMin) + 1) + 1);
            K *thr = (K *)sc.get<uint64_t>(M);
            uint32_t *tie = sc.get<uint32_t>(M);
            OSP_HIP(hipMemsetAsync(counters, 0, SELK_COUNTERS * sizeof(uint64_t), s));
            select_k_classify_kernel<K><<<grid_for(M, 256), 256, 0, s>>>(in->rowptr, M, k, kSelectKLongMin, wave_rows, long_rows, counters, thr, tie);
            launches++;
            {
                Gather g(s);
                g.add(&n_wave, (const uint64_t *)counters + SELK_NWAVE);
                g.add(&n_long, (const uint64_t *)counters + SELK_NLONG);
                g.wait();
                readbacks++;
            }
            if (n_wave + n_long == 0) {
                copy_csr<T>(in, res, s);
                return;
            }
            // ---- the pair of every capped row ----
            constexpr uint64_t kSlice = 1ull << 30;   // rows per launch (grid limit)
            for (uint64_t r0 = 0; r0 < n_wave; r0 += kSlice) {
                select_k_threshold_kernel<T, ORDER, kWave><<<(unsigned)std::min(kSlice, n_wave - r0), kWave, 0, s>>>(in->rowptr, in->colidx, val, wave_rows + r0,
                                                                                                                 k, seed, thr, tie);
                launches++;
            }
            if (n_long) {
                select_k_threshold_kernel<T, ORDER, kSelectKLongThreads><<<(unsigned)n_long, kSelectKLongThreads, 0, s>>>(in->rowptr, in->colidx, val, long_rows,
                                                                                                                      k, seed, thr, tie);
                launches++;
            }
            // ---- flag, scan, write ----
            const Compacted c = compact_by_bits<T>(sc, in, res, s, [&](unsigned nchunks, uint64_t *bits) {
                select_k_flag_kernel<T, ORDER><<<nchunks, kCompactThreads, 0, s>>>(in->rowptr, in->colidx, val, M, nnz_in, seed, thr, tie, bits);
            });
            readbacks++;
            launches += c.launches;
            nnz = c.nnz;
        });
    }
    fr.finish(res, nnz);
    *st = osp_select_k_stats_t{};
    st->nnz_in = nnz_in;
    st->nnz_out = nnz;
    st->rows_capped = n_wave + n_long;
    st->rows_long = n_long;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = readbacks;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] select_k order=%d k=%u M=%llu nnz %llu -> %llu capped=%llu long=%llu launches=%u readbacks=%u %.3f ms\n", sk.order, k,
                (unsigned long long)M, (unsigned long long)nnz_in, (unsigned long long)nnz, (unsigned long long)(n_wave + n_long),
                (unsigned long long)n_long, launches, readbacks, st->ms_total);
}

// ---- the row-wise scan of a CSR result and the weighted draws from its rows (osp_scan.h) ----
// The four steps of osp_scan.h over `in`'s rows: the entries of `src` scanned under OP into vals (nnz > 0 values, M > 0).
// Returns the kernels it launched; reads nothing back.
template <class T, int OP, class Src>
static uint32_t scan_rows(Scratch &sc, hipStream_t s, const Result *in, Src src, T *vals) {
    const uint64_t M = in->info.M, N = in->info.N, nnz = in->info.nnz_c;
    const uint64_t bound = nnz / kScanBlock + M;   // sum ceil(m_i / 32) <= this; the exact number stays on the device
    uint64_t *blkptr = sc.get<uint64_t>(M + 1);
    uint64_t *tmp = sc.get<uint64_t>(scan_scratch_entries(M));
    uint32_t launches = device_exclusive_scan<LoadRowBlocks, uint64_t>(LoadRowBlocks{in->rowptr}, M, blkptr, tmp, s);
    T *totals = sc.get<T>(bound);
    scan_local_kernel<T, OP, Src><<<grid_for(bound, kScanLocalThreads), kScanLocalThreads, 0, s>>>(in->rowptr, blkptr, M, src, vals, totals);
    launches++;
    if (std::min(N, nnz) > kScanBlock) {   // (else no row has a second block: columns are distinct)
        T *carry = sc.get<T>(bound);
        scan_chain_kernel<T, OP><<<grid_for(M, 256), 256, 0, s>>>(blkptr, M, totals, carry);
        scan_add_kernel<T, OP><<<grid_for(nnz, (unsigned)kCompactChunk), kCompactThreads, 0, s>>>(in->rowptr, blkptr, M, nnz, carry, vals);
        launches += 2;
    }
    return launches;
}

template <class T>
static void scan_impl(Context *ctx, const Result *in, Result *res, const osp_scan_t &scn, osp_scan_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, nnz = in->info.nnz_c;
    res->info = in->info;
    uint32_t launches = 0;
    if (M == 0 || nnz == 0) {
        empty_result<T>(res, M, s);
    } else {
        alloc_rowptr(res, M);
        OSP_HIP(hipMemcpyAsync(res->rowptr, in->rowptr, (M + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        alloc_entries<T>(res, nnz);
        OSP_HIP(hipMemcpyAsync(res->colidx, in->colidx, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        const Values<T> src{(T *)in->vals};   // (read only)
        T *out = (T *)res->vals;
        if (scn.op == OSP_REDUCE_PLUS) launches = scan_rows<T, RED_PLUS>(sc, s, in, src, out);
        else if (scn.op == OSP_REDUCE_MIN) launches = scan_rows<T, RED_MIN>(sc, s, in, src, out);
        else launches = scan_rows<T, RED_MAX>(sc, s, in, src, out);
    }
    fr.finish(res, nnz);
    *st = osp_scan_stats_t{};
    st->nnz_in = st->nnz_out = nnz;
    st->blocks = nnz / kScanBlock + M;
    st->ms_total = res->info.ms_total;
    st->launches = launches;
    st->readbacks = 0;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] scan op=%d M=%llu nnz=%llu blocks<=%llu launches=%u %.3f ms\n", scn.op, (unsigned long long)M, (unsigned long long)nnz,
                (unsigned long long)st->blocks, launches, st->ms_total);
}

// want_stats: the caller asked for stats, and rows_without is worth its kernel and its read-back
template <class T>
static void draw_impl(Context *ctx, const Result *in, const osp_draw_t &dr, int64_t *cols_out, int64_t *pos_out, osp_memspace_t space, bool want_stats,
                      osp_draw_stats_t *st) {
    OpFrame fr(ctx);
    hipStream_t s = fr.s;
    Scratch &sc = fr.sc;
    const uint64_t M = in->info.M, nnz = in->info.nnz_c, total = M * dr.draws;
    const bool ran = M && nnz;
    uint64_t rows_without = M;
    uint32_t launches = 0, readbacks = 0;
    // (both arrays are formed in pool buffers and copied out last: a call that fails leaves cols and pos as they were.  pos is
    // neither allocated nor written when the caller does not want it: a template parameter of the kernel)
    int64_t *cols = sc.get<int64_t>(total), *pos = pos_out ? sc.get<int64_t>(total) : nullptr;
    if (ran) {
        T *cdf = sc.get<T>(nnz);
        launches = scan_rows<T, RED_PLUS>(sc, s, in, Weights<T>{(const T *)in->vals}, cdf);
        const uint64_t s0 = select_k_mix(dr.seed + 0x9E3779B97F4A7C15ull);
        const unsigned grid = (unsigned)std::min<uint64_t>((total + 255) / 256, kDrawBlocks);   // (in 64 bits: total may be 2^40)
        if (pos) draw_kernel<T, true><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, cdf, total, dr.draws, s0, cols, pos);
        else draw_kernel<T, false><<<grid, 256, 0, s>>>(in->rowptr, in->colidx, cdf, total, dr.draws, s0, cols, pos);
        launches++;
        if (want_stats) {
            unsigned long long *without = (unsigned long long *)sc.get<uint64_t>(1);
            zero_async(s, {{without, sizeof(uint64_t)}});
            draw_without_kernel<<<(unsigned)std::min<uint64_t>(grid_for(M, 256), 256), 256, 0, s>>>(cols, M, dr.draws, without);
            launches += 2;
            rows_without = d2h((const uint64_t *)without, s);
            readbacks++;
        }
    }
    const float ms = fr.stop();
    finish_dense(s, cols, cols_out, total, space, !ran, (int64_t)-1);
    finish_dense(s, pos, pos_out, total, space, !ran, (int64_t)-1);
    if (total) OSP_HIP(hipStreamSynchronize(s));
    *st = osp_draw_stats_t{};
    st->nnz_in = nnz;
    st->nnz_out = total;
    st->rows_without = rows_without;
    st->ms_total = ms;
    st->launches = launches;
    st->readbacks = readbacks;
    if (ctx->env.verbose)
        fprintf(stderr, "[osp] draw draws=%u M=%llu nnz=%llu without=%llu launches=%u readbacks=%u %.3f ms\n", dr.draws, (unsigned long long)M,
                (unsigned long long)nnz, (unsigned long long)rows_without, launches, readbacks, st->ms_total);
}
