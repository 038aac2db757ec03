// osp_apply_mask.h -- the mask filter C<M> / C<¬M> of a CSR result (osp_csr_apply_mask,
// include/outerspace_spgemm_apply_mask.h), written for gfx950 (wave64).  DESIGN.md section 11.
//
// Keep the entries of `in` whose coordinate is (keep sense) or is not (complement sense) in a CSR pattern of the same shape.
// The flag pass of osp_compact.h's three passes: one workgroup per chunk of kAmChunk consecutive entries (a chunk may span
// rows), kAmRounds entries a lane.  An entry's row comes from chunk_entries_and_rows, its membership is a bisection for its
// column in that row of the mask.  A lane's kAmRounds searches advance together, one step of each per trip, so that many
// loads are in flight per lane: the searches are chains of dependent loads and nothing else.
// (Narrowing the search to the window of the mask row that a wave's run of same-row entries can hit was built and measured:
// MEASUREMENTS.md section 0d.  It lost on the frontier shape and changed nothing on short rows, so it is not here.)
#pragma once
#include "osp_compact.h"

namespace osp {

// this kernel's launch shape: a workgroup covers exactly one chunk of the bit array
constexpr int kAmThreads = 256;
constexpr int kAmRounds = 8;
constexpr uint64_t kAmChunk = (uint64_t)kAmThreads * kAmRounds;
static_assert(kAmThreads == kCompactThreads && kAmRounds == kCompactRounds, "the flag kernel covers one chunk of osp_compact.h");

// ---- pass 1: one verdict bit per entry ------------------------------------------------------------------------------------
// (positions in the mask and row numbers are kept in 32 bits: M and nnz(mask) are below 2^32)
__global__ __launch_bounds__(kAmThreads) void apply_mask_flag_kernel(const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                                      uint64_t M, uint64_t nnz, const int64_t *__restrict__ m_rowptr,
                                                                      const uint32_t *__restrict__ m_col, int complement,
                                                                      uint64_t *__restrict__ bits) {
    const uint64_t base = (uint64_t)blockIdx.x * kAmChunk;
    if (base >= nnz) return;
    uint32_t lo[kAmRounds], hi[kAmRounds], j[kAmRounds];
    int64_t p[kAmRounds];
    chunk_entries_and_rows(rowptr, col, M, nnz, base, p, j, lo, hi);
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const uint32_t r = lo[k] - 1;
        const bool valid = (uint64_t)p[k] < nnz;
        lo[k] = valid ? (uint32_t)m_rowptr[r] : 0u;
        hi[k] = valid ? (uint32_t)m_rowptr[r + 1] : 0u;
    }
    uint32_t end[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) end[k] = hi[k];
    bisect_together<false>(m_col, lo, hi, j);
    bool keep[kAmRounds];
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) {
        const bool member = lo[k] < end[k] && m_col[lo[k]] == j[k];
        keep[k] = (uint64_t)p[k] < nnz && member != (complement != 0);
    }
#pragma unroll
    for (int k = 0; k < kAmRounds; k++) store_verdicts(keep[k], (uint64_t)p[k], nnz, bits);
}

}  // namespace osp
