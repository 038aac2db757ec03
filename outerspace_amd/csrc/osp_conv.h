// osp_conv.h -- what a sparse LeNet does between its products (NN_models/models.py:35-84), on the device:
//   * im2col straight into CSC: the unfold matrix A that get_mtx_files.py:98-133 writes for every conv layer
//     (torch.nn.Unfold -> swapaxes(1, 2) -> reshape(-1, C*kh*kw)), so that a conv layer is the CLI's act * W^T;
//   * max-pool of a CSR activation (MaxPool2d, no padding, no dilation, floor mode).
// Activations are "pixel x channel" matrices: row n*H*W + y*W + x, column c (NHWC, the layout a product's result has).
//
// im2col.  Column k = (c, ky, kx) of A is channel c's pixel list, each pixel (n, y, x) mapped to the output row
// (n, oy, ox) with oy = (y + pad_h - ky*dil_h) / stride_h (likewise ox); pixels that land outside the output or between
// two strides are dropped.  For a fixed k the map is strictly increasing on the pixels it keeps, so an input grouped by
// channel with ascending pixels gives every column of A ascending rows as it is written: only the input (nnz_x entries)
// is sorted, never A (up to kh*kw times as many).  The unit of work is (column k, chunk of kConvChunk entries of
// channel c), one wave each -- a column per wave would be far too few waves (LeNet conv1: 25 columns).  A count pass,
// an exclusive scan over the units in column-major order and a write pass that compacts the survivors with ballot
// ranks (as bias_relu_rows_kernel does) give A in CSC.  Values are copied, never recomputed.
#pragma once
#include "osp_epilogue.h"

namespace osp {

constexpr uint32_t kConvChunk = 2048;   // input entries per unit (32 wave steps)

struct ConvGeom {
    uint32_t H, W, kh, kw, sh, sw, ph, pw, dh, dw, OH, OW;
};

// unit u -> channel c, window offset r = ky*kw + kx, chunk j of channel c.  ubase[c] = the first unit of channel c's
// first column (C+1 entries, ascending); channel c has (ubase[c+1] - ubase[c]) / khkw chunks.
struct ConvUnit {
    uint32_t c, r;
    uint64_t j;
};
__device__ __forceinline__ ConvUnit conv_unit(const uint64_t *__restrict__ ubase, uint32_t C, uint32_t khkw, uint64_t u) {
    ConvUnit cu;
    cu.c = (uint32_t)(lower_bound_dev(ubase, 0, (uint64_t)C + 1, u + 1) - 1);   // last c with ubase[c] <= u
    const uint64_t nch = (ubase[cu.c + 1] - ubase[cu.c]) / khkw, rel = u - ubase[cu.c];
    cu.r = (uint32_t)(rel / nch);
    cu.j = rel - (uint64_t)cu.r * nch;
    return cu;
}

// input pixel p -> output row of column (ky, kx); false when the pixel does not reach the output through this tap
__device__ __forceinline__ bool conv_map(const ConvGeom &g, uint32_t p, uint32_t ky, uint32_t kx, uint32_t *row) {
    const uint32_t hw = g.H * g.W;   // <= N*H*W, which fits u32 (checked on the host)
    const uint32_t n = p / hw, rem = p - n * hw, y = rem / g.W, x = rem - y * g.W;
    const int64_t ty = (int64_t)y + g.ph - (int64_t)ky * g.dh, tx = (int64_t)x + g.pw - (int64_t)kx * g.dw;
    if (ty < 0 || tx < 0) return false;
    const uint64_t oy = (uint64_t)ty / g.sh, ox = (uint64_t)tx / g.sw;
    if (oy * g.sh != (uint64_t)ty || ox * g.sw != (uint64_t)tx || oy >= g.OH || ox >= g.OW) return false;
    *row = (uint32_t)(((uint64_t)n * g.OH + oy) * g.OW + ox);
    return true;
}

// one wave per unit; pass 0 counts the unit's survivors (cnt[u]), pass 1 writes them at off[u]
template <class T, bool WRITE>
__global__ __launch_bounds__(256) void im2col_units_kernel(const int64_t *__restrict__ xptr, const uint32_t *__restrict__ xpix,
                                                           const T *__restrict__ xval, const uint64_t *__restrict__ ubase, uint32_t C,
                                                           ConvGeom g, uint64_t U, uint32_t *__restrict__ cnt,
                                                           const uint64_t *__restrict__ off, uint32_t *__restrict__ a_row,
                                                           T *__restrict__ a_val) {
    const uint64_t u = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (u >= U) return;
    const unsigned lane = lane_id();
    const ConvUnit cu = conv_unit(ubase, C, g.kh * g.kw, u);
    const uint32_t ky = cu.r / g.kw, kx = cu.r - ky * g.kw;
    const int64_t b = xptr[cu.c] + (int64_t)(cu.j * kConvChunk), ce = xptr[cu.c + 1], e = ce < b + kConvChunk ? ce : b + kConvChunk;
    uint64_t out = WRITE ? off[u] : 0ull;
    uint32_t total = 0;
    for (int64_t p0 = b; p0 < e; p0 += kWave) {
        const int64_t p = p0 + lane;
        uint32_t row = 0;
        const bool keep = p < e && conv_map(g, xpix[p], ky, kx, &row);
        const uint64_t m = __ballot(keep);
        if (WRITE && keep) {
            const uint64_t o = out + (uint64_t)__popcll(m & lanemask_lt());
            a_row[o] = row;
            a_val[o] = xval[p];
        }
        out += (uint64_t)__popcll(m);
        total += (uint32_t)__popcll(m);
    }
    if (!WRITE && lane == 0) cnt[u] = total;
}

// colptr[k] = offset of column k's first unit (k < K), colptr[K] = nnz(A)
__global__ void im2col_colptr_kernel(const uint64_t *__restrict__ ubase, const uint64_t *__restrict__ off, uint32_t C, uint32_t khkw,
                                     uint64_t U, int64_t *__restrict__ colptr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t K = (uint64_t)C * khkw;
    if (k > K) return;
    if (k == K) { colptr[K] = (int64_t)off[U]; return; }
    const uint32_t c = (uint32_t)(k / khkw), r = (uint32_t)(k - (uint64_t)c * khkw);
    const uint64_t nch = (ubase[c + 1] - ubase[c]) / khkw;
    colptr[k] = (int64_t)off[ubase[c] + (uint64_t)r * nch];
}

// ---- max-pool of a CSR activation ----
// Output row (n, py, px), every channel j: the max over the kh x kw window rows (n, py*sh + ky, px*sw + kx) of the input,
// an absent entry counting as +0 -- F.max_pool2d on the densified input.  Zeros are dropped (what csr_matrix(dense) drops).
// A window that holds a NaN gives a NaN wherever it lies, as torch does: the fold keeps the window's FIRST NaN in tap order
// (ky outer, kx inner) -- values are copied, never recomputed, so the output carries that NaN's bits -- and the entry stays
// (NaN != 0).  A window whose maximum is either zero is dropped; an all-present, all-negative window keeps its maximum.
// One wave per output row, a lane per channel, 64 channels per step; pass 0 counts, pass 1 writes (bias_relu_rows_kernel).
template <class T, bool WRITE>
__global__ __launch_bounds__(256) void csr_maxpool_rows_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                               const T *__restrict__ val, uint32_t C, uint32_t H, uint32_t W,
                                                               uint32_t PH, uint32_t PW, uint32_t kh, uint32_t kw, uint32_t sh,
                                                               uint32_t sw, uint64_t M, uint32_t *__restrict__ cnt,
                                                               const int64_t *__restrict__ out_ptr, uint32_t *__restrict__ out_col,
                                                               T *__restrict__ out_val) {
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= M) return;
    const unsigned lane = lane_id();
    const uint64_t pp = (uint64_t)PH * PW, n = r / pp, rem = r - n * pp, py = rem / PW, px = rem - py * PW;
    const uint64_t row0 = (n * H + py * sh) * W + px * sw;   // the window's top-left input row
    uint64_t out = WRITE ? (uint64_t)out_ptr[r] : 0ull;
    uint32_t total = 0;
    for (uint64_t j0 = 0; j0 < C; j0 += kWave) {
        const uint64_t j = j0 + lane;
        T v = T(0);
        if (j < C) {
            for (uint32_t ky = 0; ky < kh; ky++)
                for (uint32_t kx = 0; kx < kw; kx++) {
                    const uint64_t ir = row0 + (uint64_t)ky * W + kx;
                    const T w = csr_at(col, val, rowptr[ir], rowptr[ir + 1], (uint32_t)j);
                    // the first tap starts the fold; after it a larger value or a NaN replaces v unless v is a NaN already
                    v = (ky == 0 && kx == 0) || (v == v && !(w <= v)) ? w : v;
                }
        }
        const bool keep = j < C && v != T(0);
        const uint64_t m = __ballot(keep);
        if (WRITE && keep) {
            const uint64_t o = out + (uint64_t)__popcll(m & lanemask_lt());
            out_col[o] = (uint32_t)j;
            out_val[o] = v;
        }
        out += (uint64_t)__popcll(m);
        total += (uint32_t)__popcll(m);
    }
    if (!WRITE && lane == 0) cnt[r] = total;
}

}  // namespace osp
