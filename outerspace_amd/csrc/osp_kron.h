// osp_kron.h -- out = a (x) b, the Kronecker product of two CSR results: the kernels of osp_csr_kron
// (include/outerspace_spgemm_kron.h), written for gfx950 (wave64).  DESIGN.md section 30.
//
// The whole structure of out is closed form.  With rpA, rpB the operands' row pointers, lenA[i] = rpA[i + 1] - rpA[i]:
//   row r = ia mB + ib begins at rpA[ia] nnzB + lenA[ia] rpB[ib] and holds lenA[ia] lenB[ib] entries;
//   its q-th entry is (a's entry pa = rpA[ia] + q / lenB[ib]) x (b's entry pb = rpB[ib] + q % lenB[ib]),
//   at column colA[pa] nB + colB[pb], which ascends with q.
// Nothing is sorted, scanned, counted or read back.  Two kernels:
//   1. row pointers: a lane per row of out evaluates the first line.
//   2. entries: work is cut by OUTPUT positions, never by rows of either operand (a hub row (x) a hub row is one row of
//      millions of entries; three entries in 2^20 rows make millions of empty rows).  A workgroup takes kKronThreads *
//      kKronEntries consecutive positions, a lane kKronEntries consecutive ones: it finds the first one's (ia, ib) -- the
//      last ia with rpA[ia] nnzB <= e, then with r = e - rpA[ia] nnzB the last ib with lenA[ia] rpB[ib] <= r; both land on
//      the non-empty row among equal pointers, and both are plain searches of a row pointer for a divided target --
//      steps to the next ones (pb, then pa; when a step leaves its row of out it searches again: it never walks empty
//      rows, whose number the input chooses), and stores its columns as ONE 16-byte vector and its values as one (f32)
//      or two (f64): the stores of a wave are consecutive, 1 KiB per instruction.
//      The searches are confined between the rows of the chunk's first and last position, which every wave finds once
//      with 64 probes a step (wave_upper_bound: a scalar bisection of 2^11 rows is 11 dependent loads, and the first
//      version of this kernel spent its time waiting for 44 of them per wave); a chunk inside one row of out searches
//      nothing more.
// osp_csr_kron admits nnzA nnzB < 2^32 - 1: every position, every product of a pointer and a count below (at most
// nnz_out) and every offset inside a row of out is 32 bits wide, and so are the divisions of a search's target.
// No atomics, no LDS.  The operator is a template parameter; values that are only moved are moved as integers.
#pragma once
#include "osp_ewise.h"

namespace osp {

constexpr int kKronThreads = 256;
constexpr int kKronEntries = 4;   // output positions per lane: 16 bytes of columns
constexpr uint64_t kKronChunk = (uint64_t)kKronThreads * kKronEntries;
constexpr unsigned kKronRowBlocks = 1u << 20;   // the row pointer kernel strides over the rows with at most this many blocks
constexpr uint32_t kKronLaunches = 2;           // (OSP_KRON_LAUNCHES)

// out_rowptr[r] for r in [0, M], M = mA mB (> 0)
__global__ __launch_bounds__(256) void kron_rowptr_kernel(const int64_t *__restrict__ rpA, const int64_t *__restrict__ rpB, uint64_t M, uint32_t mB,
                                                          uint64_t nnzB, int64_t *__restrict__ out_rowptr) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= M; r += (uint64_t)gridDim.x * 256) {
        const uint32_t ia = (uint32_t)r / mB, ib = (uint32_t)r - ia * mB;   // (M < 2^32; r == M: ia = mA, ib = 0)
        const uint64_t a0 = (uint64_t)rpA[ia];
        uint64_t v = a0 * nnzB;
        if (ib) v += ((uint64_t)rpA[ia + 1] - a0) * (uint64_t)rpB[ib];      // (rpB[0] = 0: row mA of a is never read)
        out_rowptr[r] = (int64_t)v;
    }
}

// the last i in [lo, hi] with rp[i] <= x (the caller knows that rp[lo] <= x); WAVE: by the whole wave, 64 probes a step --
// every lane calls it with the same arguments
template <bool WAVE>
__device__ __forceinline__ uint32_t kron_last_at_most(const int64_t *__restrict__ rp, uint32_t lo, uint32_t hi, uint32_t x) {
    if constexpr (WAVE) return (uint32_t)(wave_upper_bound(rp, (uint64_t)lo + 1, (uint64_t)hi + 1, (int64_t)x) - 1);
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if ((uint64_t)rp[mid] <= (uint64_t)x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// Where an output position lies: its rows of a and of b, those rows' entries, and its offset q in its row of out.
struct KronPos {
    uint32_t ia, ib;
    uint32_t a0, lenA, b0, lenB;   // a's row begins at entry a0, b's at b0
    uint32_t q;
};
// Position e (< nnz_out < 2^32 - 1), whose row of a is known to lie in [ia_lo, ia_hi]; and when it is ia_lo (ia_hi), its row
// of b is known to be at least ib_lo (at most ib_hi).  rpA[ia] nnzB <= e is rpA[ia] <= e / nnzB, and lenA rpB[ib] <= r is
// rpB[ib] <= r / lenA: the pointers are searched as they are, against a target divided once.
template <bool WAVE>
__device__ __forceinline__ KronPos kron_locate(const int64_t *__restrict__ rpA, const int64_t *__restrict__ rpB, uint32_t mB, uint32_t nnzB, uint32_t e,
                                               uint32_t ia_lo, uint32_t ia_hi, uint32_t ib_lo, uint32_t ib_hi) {
    KronPos p;
    p.ia = kron_last_at_most<WAVE>(rpA, ia_lo, ia_hi, e / nnzB);
    p.a0 = (uint32_t)rpA[p.ia];
    p.lenA = (uint32_t)rpA[p.ia + 1] - p.a0;
    const uint32_t r = e - p.a0 * nnzB;   // (at most e)
    p.ib = kron_last_at_most<WAVE>(rpB, p.ia == ia_lo ? ib_lo : 0u, p.ia == ia_hi ? ib_hi : mB - 1u, r / p.lenA);
    p.b0 = (uint32_t)rpB[p.ib];
    p.lenB = (uint32_t)rpB[p.ib + 1] - p.b0;
    p.q = r - p.lenA * p.b0;
    return p;
}

// T: the value type, V: the unsigned integer of its width, OP: an EW_* from PLUS to SECOND
template <class T, int OP>
__global__ __launch_bounds__(kKronThreads) void kron_entries_kernel(const int64_t *__restrict__ rpA, const uint32_t *__restrict__ colA,
                                                                    const ValueBits<T> *__restrict__ valA, uint32_t mA,
                                                                    const int64_t *__restrict__ rpB, const uint32_t *__restrict__ colB,
                                                                    const ValueBits<T> *__restrict__ valB, uint32_t mB, uint32_t nB, uint64_t nnzB,
                                                                    uint64_t nnz_out, uint32_t *__restrict__ out_col,
                                                                    ValueBits<T> *__restrict__ out_val) {
    typedef ValueBits<T> V;
    const uint64_t base = (uint64_t)blockIdx.x * kKronChunk;
    if (base >= nnz_out) return;
    const uint64_t last = (base + kKronChunk < nnz_out ? base + kKronChunk : nnz_out) - 1;
    // the rows of the chunk's first and last position, by the whole wave (the same in every wave of the workgroup)
    const KronPos first = kron_locate<true>(rpA, rpB, mB, (uint32_t)nnzB, (uint32_t)base, 0u, mA - 1u, 0u, mB - 1u);
    const KronPos end = kron_locate<true>(rpA, rpB, mB, (uint32_t)nnzB, (uint32_t)last, first.ia, mA - 1u, first.ib, mB - 1u);
    const uint64_t e = base + (uint64_t)threadIdx.x * kKronEntries;
    if (e >= nnz_out) return;
    KronPos p = first;
    if (first.ia != end.ia || first.ib != end.ib) p = kron_locate<false>(rpA, rpB, mB, (uint32_t)nnzB, (uint32_t)e, first.ia, end.ia, first.ib, end.ib);
    else p.q += (uint32_t)(e - base);   // (the chunk lies in one row of out: nothing to search)
    uint32_t pa = p.a0 + p.q / p.lenB, pb = p.b0 + p.q % p.lenB;
    uint32_t left = p.lenA * p.lenB - p.q;   // positions from this one to the end of its row of out (<= nnz_out)
    uint32_t col[kKronEntries];
    V val[kKronEntries];
#pragma unroll
    for (int k = 0; k < kKronEntries; k++) {
        col[k] = 0u;
        val[k] = (V)0;
        if (e + k >= nnz_out) continue;
        if (k > 0) {
            if (--left == 0u) {   // the next row of out that holds an entry, however far: a search, not a walk
                p = kron_locate<false>(rpA, rpB, mB, (uint32_t)nnzB, (uint32_t)(e + k), p.ia, end.ia, p.ib, end.ib);
                pa = p.a0;
                pb = p.b0;
                left = p.lenA * p.lenB;
            } else if (++pb == p.b0 + p.lenB) {
                pb = p.b0;
                pa++;
            }
        }
        col[k] = colA[pa] * nB + colB[pb];   // (< nA nB <= 2^32 - 1)
        val[k] = ewise_apply<OP, T, V>(OP == EW_SECOND ? (V)0 : valA[pa], OP == EW_FIRST ? (V)0 : valB[pb]);
    }
    if (e + kKronEntries <= nnz_out) {   // (e is a multiple of kKronEntries, and the arrays are 16-byte aligned)
        static_assert(kKronEntries == 4, "a lane's columns are one 16-byte vector");
        *reinterpret_cast<uint4 *>(out_col + e) = make_uint4(col[0], col[1], col[2], col[3]);
        if constexpr (sizeof(V) == 4) {
            *reinterpret_cast<uint4 *>(out_val + e) = make_uint4(val[0], val[1], val[2], val[3]);
        } else {
            *reinterpret_cast<ulonglong2 *>(out_val + e) = make_ulonglong2(val[0], val[1]);
            *reinterpret_cast<ulonglong2 *>(out_val + e + 2) = make_ulonglong2(val[2], val[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kKronEntries; k++) {
            if (e + k < nnz_out) {
                out_col[e + k] = col[k];
                out_val[e + k] = val[k];
            }
        }
    }
}

}  // namespace osp
