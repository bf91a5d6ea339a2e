// R1CS check on the device (Engine::check, include/bpg.h bpg_r1cs_check): which multiplier, which constraint row does the resident witness break.
// The resident matrix is column-major (k_scalars.cuh); evaluating ROWS wants it row-major, so the first check of a circuit derives a row-major view from it -
// the mirror of k_csc_count / k_csc_fill: k_rowview_count (entries per row), the scan kernels of k_msm.cuh, k_rowview_fill ((column, coefficient slot) pairs per
// row, 8 B per entry), k_rowview_long (the list of rows too long for one lane).  One lane per ENTRY: the column of an entry is a binary search in col_ptr, and
// the constant column - O(q) entries, already in row order - goes in as one run per row (host/check.hpp rowview_entry), never through one hot counter.
// The check itself: k_check_mul (a lane per multiplier), k_check_rows (a lane per row up to `threshold` terms, 64 consecutive rows per wave, the wave's ballot
// stored as one word of the violation bitmap), k_check_rows_long (a wave per longer row, lane partials summed by shuffles, the bit set by atomicOr) and
// k_check_count (bad rows and the first of them, from the bitmap).  Scalars are Montgomery and canonical: a zero residual is eight zero words.
#pragma once
#include "../host/check.hpp"
#include "sc.cuh"

namespace bpg {

// the operand vector [a_L | a_R | a_O | v | 1] of a circuit of n multipliers and m committed values
struct CheckOperands { const scm *aL, *aR, *aO, *v; uint32_t n, m; };

#if defined(__HIPCC__)
__device__ __forceinline__ scm check_term(const CheckOperands &P, const scm *__restrict__ coef, uint2 ent) {
    const uint32_t c = ent.x;
    const scm k = coef[ent.y];
    if (c >= 3 * P.n + P.m) return k;                                               // the constant One
    const scm x = c < P.n ? P.aL[c] : c < 2 * P.n ? P.aR[c - P.n] : c < 3 * P.n ? P.aO[c - 2 * P.n] : P.v[c - 3 * P.n];
    return sc_mont_mul(k, x);
}

// ---- the row-major view.  counts: q + 1 words, zeroed
__global__ void __launch_bounds__(256) k_rowview_count(const uint32_t *__restrict__ ent_row, uint64_t const_begin, uint64_t nnz, uint32_t *__restrict__ counts) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    uint32_t row, run;
    rowview_entry(ent_row, const_begin, nnz, e, row, run);
    if (run) atomicAdd(&counts[row], run);
}
// cursor[r] = running position of row r (k_scan_apply); ent: nnz pairs (column, coefficient slot)
__global__ void __launch_bounds__(256) k_rowview_fill(const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row, const uint32_t *__restrict__ ent_coef,
                                                      uint32_t ncols, uint64_t const_begin, uint64_t nnz, uint32_t *__restrict__ cursor, uint2 *__restrict__ ent) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    uint32_t row, run;
    rowview_entry(ent_row, const_begin, nnz, e, row, run);
    if (!run) return;
    const uint32_t col = e < const_begin ? rowview_col_of(col_ptr, ncols, e) : ncols - 1;
    uint32_t pos = atomicAdd(&cursor[row], run);
    for (uint32_t k = 0; k < run; k++, pos++) ent[pos] = make_uint2(col, ent_coef[e + k]);
}
// long_rows[0] = how many rows hold more than `threshold` terms (zeroed by the caller), long_rows[1..] = those rows, in any order
__global__ void __launch_bounds__(256) k_rowview_long(const uint32_t *__restrict__ row_ptr, uint32_t q, uint32_t threshold, uint32_t *__restrict__ long_rows) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= q || !check_row_is_long(row_ptr[r + 1] - row_ptr[r], threshold)) return;
    long_rows[1 + atomicAdd(&long_rows[0], 1u)] = r;
}

// ---- the check.  report: {bad multipliers, first bad multiplier, bad rows, first bad row} as bpg_check_report has them, set to {0, none, 0, none} by the caller
__global__ void __launch_bounds__(256) k_check_mul(const scm *__restrict__ aL, const scm *__restrict__ aR, const scm *__restrict__ aO, uint32_t n,
                                                   unsigned long long *__restrict__ report) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const scm p = sc_mont_mul(aL[i], aR[i]), o = aO[i];
        uint32_t d = 0;
        BPG_UNROLL for (int k = 0; k < 8; k++) d |= p.v[k] ^ o.v[k];
        bad = d != 0;
    }
    const unsigned long long mask = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && mask) {
        atomicAdd(&report[0], (unsigned long long)__popcll(mask));
        atomicMin(&report[1], (unsigned long long)i + (unsigned long long)(__ffsll((long long)mask) - 1));
    }
}
// rows of at most `threshold` terms, one lane each; a longer row votes "fine" here and is judged by k_check_rows_long.  EVERY word of the bitmap is written.
__global__ void __launch_bounds__(256) k_check_rows(const uint32_t *__restrict__ row_ptr, const uint2 *__restrict__ ent, const scm *__restrict__ coef, CheckOperands P,
                                                    uint32_t q, uint32_t threshold, unsigned long long *__restrict__ bitmap) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (r < q) {
        const uint32_t b = row_ptr[r], e = row_ptr[r + 1];
        if (!check_row_is_long(e - b, threshold)) {
            scm acc = sc_zero();
            for (uint32_t t = b; t < e; t++) acc = sc_add(acc, check_term(P, coef, ent[t]));
            bad = !sc_iszero(acc);
        }
    }
    const unsigned long long mask = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && r < q) bitmap[check_word_of(r)] = mask;           // r is a multiple of 64 here: word r / 64 is this wave's
}
// a wave per long row: wave w of the grid takes rows w, w + waves, ... of the list; runs after k_check_rows on the same stream
__global__ void __launch_bounds__(256) k_check_rows_long(const uint32_t *__restrict__ row_ptr, const uint2 *__restrict__ ent, const scm *__restrict__ coef, CheckOperands P,
                                                         const uint32_t *__restrict__ long_rows, unsigned long long *__restrict__ bitmap) {
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t count = long_rows[0];
    for (uint32_t k = wave; k < count; k += waves) {                               // (k, count and the row are the same in every lane of a wave)
        const uint32_t r = long_rows[1 + k], b = row_ptr[r], e = row_ptr[r + 1];
        scm acc = sc_zero();
        for (uint32_t t = b + lane; t < e; t += 64) acc = sc_add(acc, check_term(P, coef, ent[t]));
        for (uint32_t off = 32; off > 0; off >>= 1) {
            scm o;
            BPG_UNROLL for (int i = 0; i < 8; i++) o.v[i] = __shfl_down(acc.v[i], off, 64);
            acc = sc_add(acc, o);
        }
        if (lane == 0 && !sc_iszero(acc)) atomicOr(&bitmap[check_word_of(r)], (unsigned long long)check_bit_of(r));
    }
}
// bad rows and the first of them: a lane per word of the bitmap
__global__ void __launch_bounds__(256) k_check_count(const unsigned long long *__restrict__ bitmap, uint32_t nwords, unsigned long long *__restrict__ report) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long x = w < nwords ? bitmap[w] : 0ull;
    const unsigned long long any = __ballot(x != 0);
    if (!any) return;                                                               // (the same in every lane of the wave)
    uint32_t cnt = (uint32_t)__popcll(x);
    for (uint32_t off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    const uint32_t lane = threadIdx.x & 63;
    if (lane == 0) atomicAdd(&report[2], (unsigned long long)cnt);
    if (lane == (uint32_t)(__ffsll((long long)any) - 1)) atomicMin(&report[3], (unsigned long long)w * 64 + (unsigned long long)(__ffsll((long long)x) - 1));
}
#endif  // __HIPCC__

}  // namespace bpg
