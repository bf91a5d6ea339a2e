// TEST HARNESS, stand-alone: the host half of the R1CS check (csrc/host/check.hpp) through the host compiler.  tests/test_check_host.py builds it with
// -fsanitize=address,undefined and expects "ok" on the last line.
//   1. The row-major view as the kernels k_rowview_count / k_rowview_fill / k_rowview_long derive it from the column-major matrix - every entry once, through
//      rowview_entry and rowview_col_of - on matrices with empty rows, empty columns, rows of several constant terms and rows around the long-row threshold, into
//      buffers of EXACTLY the sizes the formulas give; every row of the view must hold the row's terms (as a multiset of (column, coefficient slot)).
//   2. The violation bitmap: check_word_of / check_bit_of against a set of rows, and check_bitmap_rows piece by piece as Engine::check reads it back (a piece that
//      ends inside the list, a cap below and above the count, bits past q ignored).
//   3. check_host on a small instance with every variable kind, satisfied and broken one row / one multiplier at a time.
#include "../../bulletproofs_gadgets_amd/csrc/host/check.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>
using namespace bpg;

static int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

struct Term { uint32_t col, coef; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t mod) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33) % mod; }

// rows over ncols columns (the last one the constants) -> the column-major form upload() leaves: variable columns in index order, entries of a column in row
// order; the constant column laid out row after row
static int check_view(const std::vector<std::vector<Term>> &rows, uint32_t ncols, uint32_t threshold) {
    const uint64_t q = rows.size();
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> cols(ncols);
    for (uint32_t r = 0; r < q; r++) for (const Term &t : rows[r]) cols.at(t.col).push_back({r, t.coef});
    uint64_t nnz = 0;
    for (auto &c : cols) nnz += c.size();
    // heap buffers of exactly the sizes the engine allocates for the matrix
    std::unique_ptr<uint64_t[]> col_ptr(new uint64_t[ncols + 1]);
    std::unique_ptr<uint32_t[]> ent_row(new uint32_t[nnz ? nnz : 1]), ent_coef(new uint32_t[nnz ? nnz : 1]);
    uint64_t e = 0;
    for (uint32_t c = 0; c < ncols; c++) { col_ptr[c] = e; for (auto &x : cols[c]) { ent_row[e] = x.first; ent_coef[e] = x.second; e++; } }
    col_ptr[ncols] = e;
    const uint64_t const_begin = col_ptr[ncols - 1];
    // every entry's column by the search
    for (uint32_t c = 0; c < ncols; c++) for (uint64_t k = col_ptr[c]; k < col_ptr[c + 1]; k++) if (rowview_col_of(col_ptr.get(), ncols, k) != c) return fail("rowview_col_of");
    // the runs of the constant column cover it exactly once
    uint64_t covered = 0;
    for (uint64_t k = const_begin; k < nnz; k++) { uint32_t row, run; rowview_entry(ent_row.get(), const_begin, nnz, k, row, run); if (run && covered != k - const_begin) return fail("constant runs overlap"); covered += run; }
    if (covered != nnz - const_begin) return fail("constant runs do not cover the column");
    const RowViewHost V = rowview_build_host(col_ptr.get(), ent_row.get(), ent_coef.get(), ncols, q, const_begin, nnz, threshold);
    if (V.row_ptr.size() != q + 1 || V.row_ptr[q] != nnz) return fail("row_ptr");
    std::vector<uint32_t> want_long;
    for (uint32_t r = 0; r < q; r++) {
        std::vector<std::pair<uint32_t, uint32_t>> got, want;
        for (uint32_t k = V.row_ptr[r]; k < V.row_ptr[r + 1]; k++) got.push_back({V.ent_col.at(k), V.ent_coef.at(k)});
        for (const Term &t : rows[r]) want.push_back({t.col, t.coef});
        std::sort(got.begin(), got.end()); std::sort(want.begin(), want.end());
        if (got != want) return fail("a row of the view differs from the row");
        if (rows[r].size() > threshold) want_long.push_back(r);
    }
    if (V.long_rows != want_long) return fail("long rows");
    return 0;
}

static int check_views() {
    // by hand: n = 2, m = 1 -> columns 0..5 left, right, output, 6 committed, 7 constants; an empty row, an empty column (3), two constants in one row
    const std::vector<std::vector<Term>> small = {
        {{0, 1}, {2, 2}, {7, 0}}, {}, {{7, 3}, {6, 1}, {7, 4}}, {{7, 5}}, {{1, 1}, {4, 2}, {5, 2}, {6, 0}}, {}, {{7, 1}, {7, 1}, {7, 2}, {0, 9}},
    };
    for (uint32_t th : {0u, 1u, 2u, 3u, 4u, 100u}) if (check_view(small, 8, th)) return 1;
    if (check_view({}, 1, 4)) return 1;                                            // q = 0, no variable at all
    if (check_view({{}, {}}, 1, 4)) return 1;                                      // rows without terms
    if (check_view({{{0, 0}}}, 1, 4)) return 1;                                    // one constant-only row
    // random: 300 rows over 40 columns, lengths 0..70 around a threshold of 64, a few rows over every column
    std::vector<std::vector<Term>> big(300);
    for (uint32_t r = 0; r < big.size(); r++) {
        const uint32_t len = r % 50 == 7 ? 40 : rnd(4) == 0 ? 62 + rnd(6) : rnd(6);
        for (uint32_t k = 0; k < len; k++) big[r].push_back({r % 50 == 7 ? k : (rnd(3) == 0 ? 39u : rnd(39)), rnd(17)});
    }
    for (uint32_t th : {0u, 63u, 64u, 65u}) if (check_view(big, 40, th)) return 1;
    return 0;
}

static int check_bitmap() {
    const uint64_t q = 1000;
    std::vector<uint64_t> bad = {0, 1, 63, 64, 65, 127, 128, 500, 640, 959, 960, 999};
    const uint64_t nwords = check_bitmap_words(q);
    if (nwords != 16 || check_bitmap_words(0) != 0 || check_bitmap_words(64) != 1 || check_bitmap_words(65) != 2) return fail("check_bitmap_words");
    std::unique_ptr<uint64_t[]> words(new uint64_t[nwords]);
    std::memset(words.get(), 0, nwords * 8);
    for (uint64_t r : bad) words[check_word_of(r)] |= check_bit_of(r);
    words[15] |= check_bit_of(1010);                                               // a bit past q: never reported
    for (uint64_t cap : {0ull, 1ull, 5ull, 12ull, 40ull}) {
        for (uint64_t piece : {1ull, 3ull, 16ull}) {
            const uint64_t want = std::min<uint64_t>(cap, bad.size());
            std::unique_ptr<uint64_t[]> out(new uint64_t[want ? want : 1]);
            uint64_t have = 0;
            for (uint64_t w0 = 0; w0 < nwords && have < want; w0 += piece)
                have = check_bitmap_rows(words.get() + w0, std::min(piece, nwords - w0), w0, q, want, out.get(), have);
            if (have != want) return fail("check_bitmap_rows: count");
            for (uint64_t k = 0; k < have; k++) if (out[k] != bad[k]) return fail("check_bitmap_rows: rows");
        }
    }
    // from the word of the first bad row on, as Engine::check reads it
    std::unique_ptr<uint64_t[]> out(new uint64_t[3]);
    const uint64_t w0 = check_word_of(500);
    std::vector<uint64_t> tail(words.get() + w0, words.get() + nwords);
    tail[0] &= ~(check_bit_of(500) - 1);
    if (check_bitmap_rows(tail.data(), tail.size(), w0, q, 3, out.get(), 0) != 3 || out[0] != 500 || out[1] != 640 || out[2] != 959) return fail("check_bitmap_rows: from a later word");
    return 0;
}

static void put(std::vector<uint8_t> &v, uint64_t x) { uint8_t b[32] = {0}; std::memcpy(b, &x, 8); v.insert(v.end(), b, b + 32); }
static void put(std::vector<uint8_t> &v, const Scalar &s) { uint8_t b[32]; s.to_bytes(b); v.insert(v.end(), b, b + 32); }

static int check_definition() {
    // n = 2: 3 * 4 = 12, 5 * 6 = 30; m = 1: v = 7.  coef: 0 -> 1, 1 -> -1, 2 -> 2, 3 -> -30, 4 -> 5
    FlatCircuit f; f.n = 2; f.m = 1;
    for (uint64_t x : {3, 5}) put(f.aL, x);
    for (uint64_t x : {4, 6}) put(f.aR, x);
    for (uint64_t x : {12, 30}) put(f.aO, x);
    put(f.coef, (uint64_t)1); put(f.coef, -Scalar::one()); put(f.coef, (uint64_t)2); put(f.coef, -Scalar::from_u64(30)); put(f.coef, (uint64_t)5);
    auto V = [](uint32_t kind, uint32_t idx) { return kind << 29 | idx; };
    const std::vector<std::vector<std::pair<uint32_t, uint32_t>>> rows = {
        {{V(2, 1), 0}, {V(4, 0), 3}},                        // aO[1] - 30 = 0
        {},                                                  // 0 = 0
        {{V(0, 0), 0}, {V(1, 0), 0}, {V(3, 0), 1}},          // aL[0] + aR[0] - v = 0
        {{V(2, 0), 2}, {V(2, 1), 1}, {V(1, 1), 1}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}, {V(4, 0), 0}},   // 24 - 30 - 6 + 12 = 0
        {{V(0, 1), 4}, {V(3, 0), 1}, {V(4, 0), 0}},          // 25 - 7 + 1 != 0
    };
    for (auto &r : rows) { for (auto &t : r) { f.term_var.push_back(t.first); f.term_coef.push_back(t.second); } f.row_ptr.push_back(f.term_var.size()); }
    std::vector<uint8_t> v; put(v, (uint64_t)7);
    std::unique_ptr<uint64_t[]> out(new uint64_t[2]);
    uint64_t have = 9;
    CheckReport R = check_host(FlatView(f), v.data(), 2, out.get(), &have);
    if (R.bad_multipliers != 0 || R.first_bad_multiplier != CHECK_NONE || R.bad_rows != 1 || R.first_bad_row != 4 || have != 1 || out[0] != 4) return fail("check_host: the instance as it stands");
    std::vector<uint8_t> v2; put(v2, (uint64_t)8);           // v = 8: row 2 breaks too
    R = check_host(FlatView(f), v2.data(), 1, out.get(), &have);
    if (R.bad_rows != 2 || R.first_bad_row != 2 || have != 1 || out[0] != 2) return fail("check_host: a bumped committed value");
    R = check_host(FlatView(f), v2.data(), 0, nullptr, &have);
    if (R.bad_rows != 2 || have != 0) return fail("check_host: cap 0");
    f.aO[32] ^= 1;                                           // aO[1] = 31: multiplier 1, rows 0 and 3
    R = check_host(FlatView(f), v.data(), 2, out.get(), &have);
    if (R.bad_multipliers != 1 || R.first_bad_multiplier != 1 || R.bad_rows != 3 || R.first_bad_row != 0 || have != 2 || out[0] != 0 || out[1] != 3) return fail("check_host: a bumped output");
    return 0;
}

int main() {
    if (check_views()) return 1;
    std::printf("views ok\n");
    if (check_bitmap()) return 1;
    std::printf("bitmap ok\n");
    if (check_definition()) return 1;
    std::printf("definition ok\nok\n");
    return 0;
}
