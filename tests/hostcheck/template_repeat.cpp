// TEST HARNESS, stand-alone: compiles the index map of a repeated template and the repeat-layout witness interpreter (csrc/hip/k_repeat.cuh, the BPG_HD half,
// over csrc/hip/k_witness.cuh) for the host.  tests/test_template_repeat_host.py builds it with -fsanitize=address,undefined and expects "ok" on the last line.
//   1. The column-major replication as the kernels k_repeat_colptr / k_repeat_entries do it - every (column, copy) and (entry, copy) once, through repeat_map,
//      repeat_col_of, repeat_var_of and repeat_entry_pos - on a small matrix with every section (left, right, output, committed, constants) and a parameter
//      slot, into heap buffers of EXACTLY the sizes the formulas give; the result is compared with the transpose of the row-major repeat made term by term.
//   2. witness_eval_repeat_lane over a hand-packed program of two segments (a product chain and a run of bit hints over a committed value), n = 5 (no
//      power of two), K = 67 items: item k's vectors at k n, its committed values at k m, compared with plain integer arithmetic.
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_repeat.cuh"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>
using namespace bpg;

static int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

struct Term { uint32_t var, coef; };
static uint32_t V(uint32_t kind, uint32_t idx) { return kind << 29 | idx; }

static int check_matrix(uint32_t K) {
    // source: n = 3, m = 2, q = 4, shared coefficients [0, 4), one parameter slot (4) on row 3
    const RepeatDims D{3, 2, 4, 4, 1};
    const std::vector<std::vector<Term>> rows = {
        {{V(0, 0), 1}, {V(1, 2), 2}, {V(4, 0), 0}},
        {{V(2, 1), 3}, {V(3, 0), 1}, {V(0, 0), 2}},
        {{V(3, 1), 0}, {V(1, 1), 1}, {V(4, 0), 3}, {V(2, 2), 2}},
        {{V(2, 2), 1}, {V(3, 1), 2}, {V(4, 0), 4}},
    };
    // column-major form of a row list: per column the (row, coef) entries; columns sorted, entries in row order
    auto transpose = [](const std::vector<std::vector<Term>> &R, uint32_t n, uint32_t m, std::vector<uint64_t> &cp, std::vector<uint32_t> &er, std::vector<uint32_t> &ec) {
        const uint32_t ncol = 3 * n + m + 1;
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> cols(ncol);
        for (uint32_t r = 0; r < R.size(); r++) for (const Term &t : R[r]) cols[repeat_col_of(t.var, n, m)].push_back({r, t.coef});
        cp.assign(1, 0); er.clear(); ec.clear();
        for (auto &c : cols) { for (auto &e : c) { er.push_back(e.first); ec.push_back(e.second); } cp.push_back(er.size()); }
    };
    std::vector<uint64_t> cp; std::vector<uint32_t> er, ec;
    transpose(rows, D.n, D.m, cp, er, ec);
    const uint64_t nnz = er.size();
    // the yardstick: the row-major repeat, term by term, transposed
    std::vector<std::vector<Term>> rep(K * rows.size());
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t r = 0; r < rows.size(); r++)
            for (const Term &t : rows[r]) {
                uint32_t var, coef, row;
                repeat_map(D, k, t.var, t.coef, r, var, coef, row);
                if (row >= rep.size()) return fail("row out of range");
                rep[row].push_back({var, coef});
            }
    std::vector<uint64_t> wcp; std::vector<uint32_t> wer, wec;
    transpose(rep, K * D.n, K * D.m, wcp, wer, wec);
    // the replication on columns, as the kernels do it, into exact-size heap buffers
    const uint32_t ncol = 3 * D.n + D.m;
    std::vector<uint64_t> out((size_t)3 * K * D.n + K * D.m + 2, ~0ull);
    std::vector<uint32_t> orow(K * nnz, ~0u), ocoef(K * nnz, ~0u);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c <= ncol; c++) {
            if (c == ncol) { if (k == 0) { out[3 * K * D.n + K * D.m] = K * cp[ncol]; out[3 * K * D.n + K * D.m + 1] = K * cp[ncol + 1]; } continue; }
            const uint32_t sec = c < 3 * D.n ? c / D.n : 3u, c0 = sec * D.n, c1 = sec < 3 ? c0 + D.n : c0 + D.m;
            uint32_t var, coef, row;
            repeat_map(D, k, repeat_var_of(c, D.n, D.m), 0, 0, var, coef, row);
            out.at(repeat_col_of(var, K * D.n, K * D.m)) = repeat_entry_pos(K, k, cp[c0], cp[c1], cp[c]);
        }
    const uint64_t b[6] = {0, cp[D.n], cp[2 * D.n], cp[3 * D.n], cp[3 * D.n + D.m], nnz};
    for (uint32_t k = 0; k < K; k++)
        for (uint64_t e = 0; e < nnz; e++) {
            int s = 0; while (e >= b[s + 1]) s++;
            uint32_t var, coef, row;
            repeat_map(D, k, 4u << 29, ec[e], er[e], var, coef, row);
            const uint64_t pos = repeat_entry_pos(K, k, b[s], b[s + 1], e);
            if (orow.at(pos) != ~0u) return fail("two entries at one position");
            orow[pos] = row; ocoef[pos] = coef;
        }
    if (out != wcp) return fail("col_ptr of the repeat");
    // entries of a column may come in another order than the transpose's (copy-major in the constant column): compare per column as sets
    for (size_t c = 0; c + 1 < out.size(); c++) {
        std::vector<std::pair<uint32_t, uint32_t>> a, w;
        for (uint64_t e = out[c]; e < out[c + 1]; e++) { a.push_back({orow[e], ocoef[e]}); w.push_back({wer[e], wec[e]}); }
        std::sort(a.begin(), a.end()); std::sort(w.begin(), w.end());
        if (a != w) return fail("entries of a column");
    }
    return 0;
}

static scm small(uint32_t x) { uint32_t w[8] = {x, 0, 0, 0, 0, 0, 0, 0}; return sc_from_words(w); }
static uint64_t low64(const scm &s) { uint32_t w[8]; sc_to_words(w, s); for (int i = 2; i < 8; i++) if (w[i]) return ~0ull; return (uint64_t)w[1] << 32 | w[0]; }

static int check_interpreter(uint32_t K) {
    // n = 5, m = 2.  Segment A (multipliers 0, 1): a0 = (v0 + 3) * v0; a1 = o0 * (l0 - 1)   [left list = right list for none].
    // Segment B (multipliers 2, 3, 4): bits 0, 1, 5 of v1 (hints; the second and third share the source).
    const uint32_t n = 5, m = 2;
    const std::vector<scm> coef = {small(3), small(1)};         // slot 0: general 3; slot 1 is never read (classes +1 / -1 need no table)
    auto cw = [](uint32_t cls, uint32_t idx) { return cls << WIT_CLASS_SHIFT | idx; };
    const std::vector<uint32_t> stream = {
        /* mul 0 */ 2, 1, V(3, 0), cw(WIT_COEF_PLUS_ONE, 1), V(4, 0), cw(WIT_COEF_GENERAL, 0), V(3, 0), cw(WIT_COEF_PLUS_ONE, 1),
        /* mul 1 */ 1, 2, V(2, 0), cw(WIT_COEF_PLUS_ONE, 1), V(0, 0), cw(WIT_COEF_PLUS_ONE, 1), V(4, 0), cw(WIT_COEF_MINUS_ONE, 1),
        /* mul 2 */ 1, WIT_HINT_BIT_PAIR | 0, V(3, 1), cw(WIT_COEF_PLUS_ONE, 1),
        /* mul 3 */ 0, WIT_HINT_BIT_PAIR | WIT_HINT_SAME_SOURCE | 1,
        /* mul 4 */ 0, WIT_HINT_BIT_PAIR | WIT_HINT_SAME_SOURCE | 5,
    };
    const uint32_t segA[3] = {0, 2, 0}, segB[3] = {2, 3, 16};
    std::vector<scm> v((size_t)K * m), aL((size_t)K * n), aR((size_t)K * n), aO((size_t)K * n);   // exact sizes: item K - 1 ends at the last element
    for (uint32_t k = 0; k < K; k++) { v[(size_t)k * m] = small(10 + k); v[(size_t)k * m + 1] = small(37 * k + 6); }
    for (const uint32_t *sg : {segA, segB})
        for (uint32_t k = 0; k < K; k++) witness_eval_repeat_lane(sg[0], sg[1], stream.data() + sg[2], coef.data(), v.data(), n, m, k, aL.data(), aR.data(), aO.data());
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t v0 = 10 + k, v1 = 37 * k + 6, l0 = v0 + 3, o0 = l0 * v0;
        const uint64_t wl[5] = {l0, o0, 1 - (v1 & 1), 1 - ((v1 >> 1) & 1), 1 - ((v1 >> 5) & 1)};
        const uint64_t wr[5] = {v0, l0 - 1, v1 & 1, (v1 >> 1) & 1, (v1 >> 5) & 1};
        const uint64_t wo[5] = {o0, o0 * (l0 - 1), 0, 0, 0};
        for (uint32_t i = 0; i < n; i++)
            if (low64(aL[(size_t)k * n + i]) != wl[i] || low64(aR[(size_t)k * n + i]) != wr[i] || low64(aO[(size_t)k * n + i]) != wo[i]) {
                std::printf("item %u multiplier %u\n", k, i);
                return fail("interpreter");
            }
    }
    return 0;
}

int main() {
    for (uint32_t K : {1u, 2u, 3u, 67u}) if (check_matrix(K)) return 1;
    if (check_interpreter(1) || check_interpreter(67)) return 1;
    std::printf("ok\n");
    return 0;
}
