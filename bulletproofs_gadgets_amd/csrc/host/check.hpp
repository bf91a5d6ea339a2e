// "Is this witness satisfying, and if not, where does it fail" (include/bpg.h bpg_r1cs_check): the definition, and the bookkeeping the device path shares.
//   multiplier i is BAD when a_L[i] * a_R[i] != a_O[i];  constraint row j is BAD when sum over its terms of coef * value != 0 (mod l), the value of a term
//   read from the operand vector [a_L | a_R | a_O | v | 1] at the term's column (left i -> i, right i -> n + i, output i -> 2n + i, committed j -> 3n + j,
//   One -> 3n + m: the columns of the resident matrix, hip/k_scalars.cuh).
// check_host() is that definition on a row-major instance in host scalars - the device-less mirror (bpg_test_check_host) the GPU tests compare against.
// The BPG_CHECK_HD half is what hip/k_check.cuh runs per lane and tests/hostcheck/check_rows.cpp runs under the sanitizers: where an entry of the column-major
// matrix goes in the row-major view (rowview_entry), the bit of a row in the violation bitmap, and the bitmap-to-list extraction.  No HIP in this file.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "r1cs.hpp"
#include "scalar.hpp"

// shared with the kernels (the compiler's own attribute spelling: this header is read before any HIP header in host-side translation units)
#if defined(__HIPCC__)
#define BPG_CHECK_HD __attribute__((host)) __attribute__((device)) inline
#else
#define BPG_CHECK_HD inline
#endif

namespace bpg {

constexpr uint64_t CHECK_NONE = ~(uint64_t)0;       // first_bad_* when there is none
// Rows of at most this many terms are summed by ONE lane (64 consecutive rows per wave); longer rows by a whole wave each (k_check_rows_long).
// Measured, not derived ("R1CS check on the device"); BPG_CHECK_THRESHOLD overrides it per context.
constexpr uint32_t CHECK_ROW_THRESHOLD = 128;

struct CheckReport {            // = bpg_check_report
    uint64_t bad_multipliers = 0, first_bad_multiplier = CHECK_NONE, bad_rows = 0, first_bad_row = CHECK_NONE;
};

// ---- the violation bitmap: one bit per row, 64 consecutive rows per word (the ballot of the wave that summed them)
BPG_CHECK_HD uint64_t check_bitmap_words(uint64_t q) { return (q + 63) / 64; }
BPG_CHECK_HD uint64_t check_word_of(uint64_t row) { return row >> 6; }
BPG_CHECK_HD uint64_t check_bit_of(uint64_t row) { return (uint64_t)1 << (row & 63); }
BPG_CHECK_HD bool check_row_is_long(uint32_t terms, uint32_t threshold) { return terms > threshold; }

// ---- the row-major view from the column-major matrix (col_ptr: ncols + 1 entries, the constant column last; entries = (row, coefficient slot))
// column of entry e: the last column c with col_ptr[c] <= e (empty columns share their start with the next one and are skipped)
BPG_CHECK_HD uint32_t rowview_col_of(const uint64_t *col_ptr, uint32_t ncols, uint64_t e) {
    uint32_t lo = 0, hi = ncols;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (col_ptr[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}
// What the lane of entry e adds to its row: `run` entries [e, e + run) of row `row`.  An entry of a variable column is a run of one.  The constant column can
// hold O(q) entries and is already in row order (upload lays it out by a scan over the rows, a repeat writes copy after copy): the FIRST entry of a run of
// equal rows carries the whole run, the others carry nothing - one addition per row, whatever the row holds.
BPG_CHECK_HD void rowview_entry(const uint32_t *ent_row, uint64_t const_begin, uint64_t nnz, uint64_t e, uint32_t &row, uint32_t &run) {
    row = ent_row[e]; run = 1;
    if (e < const_begin) return;
    if (e > const_begin && ent_row[e - 1] == row) { run = 0; return; }
    while (e + run < nnz && ent_row[e + run] == row) run++;
}

// ---- bitmap -> list: the set bits of words[0, nwords) as rows word0 * 64 + ..., ascending, appended to rows_out until it holds cap; returns the new count
inline uint64_t check_bitmap_rows(const uint64_t *words, uint64_t nwords, uint64_t word0, uint64_t q, uint64_t cap, uint64_t *rows_out, uint64_t have) {
    for (uint64_t w = 0; w < nwords && have < cap; w++) {
        uint64_t x = words[w];
        while (x && have < cap) {
            const uint64_t row = (word0 + w) * 64 + (uint64_t)__builtin_ctzll(x);
            x &= x - 1;
            if (row < q) rows_out[have++] = row;
        }
    }
    return have;
}

// ---- the view on the host, by the same per-entry steps the kernels take (k_rowview_count, the scan, k_rowview_fill, k_rowview_long)
struct RowViewHost {
    std::vector<uint32_t> row_ptr;              // q + 1
    std::vector<uint32_t> ent_col, ent_coef;    // per row, in any order
    std::vector<uint32_t> long_rows;            // rows of more than `threshold` terms
};
inline RowViewHost rowview_build_host(const uint64_t *col_ptr, const uint32_t *ent_row, const uint32_t *ent_coef, uint32_t ncols, uint64_t q, uint64_t const_begin,
                                      uint64_t nnz, uint32_t threshold) {
    RowViewHost V;
    std::vector<uint32_t> counts(q + 1, 0);
    for (uint64_t e = 0; e < nnz; e++) { uint32_t row, run; rowview_entry(ent_row, const_begin, nnz, e, row, run); counts.at(row) += run; }
    V.row_ptr.assign(q + 1, 0);
    for (uint64_t r = 0; r < q; r++) V.row_ptr[r + 1] = V.row_ptr[r] + counts[r];
    std::vector<uint32_t> cursor(V.row_ptr.begin(), V.row_ptr.end() - 1);
    V.ent_col.assign(nnz, 0); V.ent_coef.assign(nnz, 0);
    for (uint64_t e = 0; e < nnz; e++) {
        uint32_t row, run; rowview_entry(ent_row, const_begin, nnz, e, row, run);
        if (!run) continue;
        const uint32_t col = e < const_begin ? rowview_col_of(col_ptr, ncols, e) : ncols - 1;
        uint32_t pos = cursor.at(row); cursor[row] += run;
        for (uint32_t k = 0; k < run; k++, pos++) { V.ent_col.at(pos) = col; V.ent_coef.at(pos) = ent_coef[e + k]; }
    }
    for (uint64_t r = 0; r < q; r++) if (check_row_is_long(V.row_ptr[r + 1] - V.row_ptr[r], threshold)) V.long_rows.push_back((uint32_t)r);
    return V;
}

// ---- the definition on a row-major instance (the mirror).  The caller has checked the instance (Engine::check_instance) and that it carries a witness;
// v: m x 32 bytes, reduced mod l as assign() reduces them.  rows_out receives the lowest min(cap, bad_rows) bad rows, ascending.
inline CheckReport check_host(const FlatView &c, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out) {
    CheckReport R;
    auto load = [](const uint8_t *p, uint64_t count) { std::vector<Scalar> out(count); for (uint64_t i = 0; i < count; i++) out[i] = Scalar::from_bytes_mod_order(p + 32 * i); return out; };
    const std::vector<Scalar> aL = load(c.aL, c.n), aR = load(c.aR, c.n), aO = load(c.aO, c.n), vv = load(v, c.m), coef = load(c.coef, c.ncoef);
    for (uint64_t i = 0; i < c.n; i++)
        if (aL[i] * aR[i] != aO[i]) { if (!R.bad_multipliers++) R.first_bad_multiplier = i; }
    uint64_t have = 0;
    for (uint64_t r = 0; r < c.q; r++) {
        Scalar acc;
        for (uint64_t t = c.row_ptr[r]; t < c.row_ptr[r + 1]; t++) {
            const uint32_t kind = c.term_var[t] >> 29, idx = c.term_var[t] & 0x1fffffffu;
            const Scalar &k = coef[c.term_coef[t]];
            acc += kind == 0 ? k * aL[idx] : kind == 1 ? k * aR[idx] : kind == 2 ? k * aO[idx] : kind == 3 ? k * vv[idx] : k;
        }
        if (acc != Scalar::zero()) {
            if (!R.bad_rows++) R.first_bad_row = r;
            if (have < cap) rows_out[have++] = r;
        }
    }
    if (n_rows_out) *n_rows_out = have;
    return R;
}

}  // namespace bpg
