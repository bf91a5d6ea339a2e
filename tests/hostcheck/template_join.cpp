// TEST HARNESS, stand-alone: compiles the index map of joined templates and the join-layout witness interpreter (csrc/hip/k_join.cuh, the BPG_HD half, over
// csrc/hip/k_repeat.cuh and csrc/hip/k_witness.cuh) for the host.  tests/test_template_join_host.py builds it with -fsanitize=address,undefined and expects "ok"
// on the last line.  For several part lists over three small templates (every section, shared coefficients, parameter slots, one template without any):
//   1. join_map is injective on variables, rows and coefficient slots and lands inside the totals; the slots form one range behind the shared parts.
//   2. The column-major replication as the kernels k_join_colptr / k_join_entries / k_join_coef do it - every (part, column, copy) and (part, entry, copy) once -
//      into heap buffers of EXACTLY the sizes the formulas give: the entry positions are a bijection onto [0, nnz'), the column pointers are monotone, and the
//      result is the transpose of the row-major join made term by term; the constants column is in ascending row order.
//   3. A join of one part equals repeat_map / repeat_entry_pos term for term.
//   4. witness_eval_join_lane and join_ck_place over a hand-packed program in two parts of different shapes, 67 and 3 items, against plain integers.
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_join.cuh"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
using namespace bpg;

static int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

struct Term { uint32_t var, coef; };
static uint32_t V(uint32_t kind, uint32_t idx) { return kind << 29 | idx; }
using Rows = std::vector<std::vector<Term>>;
struct Source { uint32_t n, m, shared, n_params; Rows rows; };

static const Source kSources[3] = {
    // n = 3, m = 2, q = 4, shared coefficients [0, 4), one parameter slot (4) on row 3
    {3, 2, 4, 1, {{{V(0, 0), 1}, {V(1, 2), 2}, {V(4, 0), 0}},
                  {{V(2, 1), 3}, {V(3, 0), 1}, {V(0, 0), 2}},
                  {{V(3, 1), 0}, {V(1, 1), 1}, {V(4, 0), 3}, {V(2, 2), 2}},
                  {{V(2, 2), 1}, {V(3, 1), 2}, {V(4, 0), 4}}}},
    // n = 2, m = 1, q = 2, shared [0, 2), no parameter, no constant term
    {2, 1, 2, 0, {{{V(0, 1), 0}, {V(3, 0), 1}}, {{V(1, 0), 1}, {V(2, 1), 0}, {V(0, 0), 1}}}},
    // n = 1, m = 0, q = 2, NO shared coefficient, two parameter slots
    {1, 0, 0, 2, {{{V(0, 0), 0}, {V(4, 0), 1}}, {{V(2, 0), 1}, {V(4, 0), 0}}}},
};

// column-major form of a row list: per column the (row, coef) entries; columns sorted, entries in row order
static void transpose(const Rows &R, uint32_t n, uint32_t m, std::vector<uint64_t> &cp, std::vector<uint32_t> &er, std::vector<uint32_t> &ec) {
    const uint32_t ncol = 3 * n + m + 1;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> cols(ncol);
    for (uint32_t r = 0; r < R.size(); r++) for (const Term &t : R[r]) cols[repeat_col_of(t.var, n, m)].push_back({r, t.coef});
    cp.assign(1, 0); er.clear(); ec.clear();
    for (auto &c : cols) { for (auto &e : c) { er.push_back(e.first); ec.push_back(e.second); } cp.push_back(er.size()); }
}

struct PartSpec { int src; uint32_t count; };

static int check_matrix(const std::vector<PartSpec> &spec) {
    const size_t np = spec.size();
    std::vector<JoinPart> parts(np);
    std::vector<std::vector<uint64_t>> cps(np);
    std::vector<std::vector<uint32_t>> ers(np), ecs(np);
    for (size_t p = 0; p < np; p++) {
        const Source &S = kSources[spec[p].src];
        transpose(S.rows, S.n, S.m, cps[p], ers[p], ecs[p]);
        JoinPart &P = parts[p];
        std::memset(&P, 0, sizeof P);
        P.n = S.n; P.m = S.m; P.q = (uint32_t)S.rows.size(); P.shared = S.shared; P.n_params = S.n_params; P.n_ck = 0; P.count = spec[p].count;
        const uint64_t b[6] = {0, cps[p][S.n], cps[p][2 * S.n], cps[p][3 * S.n], cps[p][3 * S.n + S.m], ers[p].size()};
        std::memcpy(P.sec, b, sizeof b);
    }
    const JoinTotals T = join_fill_bases(parts.data(), np);
    const uint64_t ncoef = T.shared + T.n_params;
    // 1. the map, term by term: the row-major join (the yardstick of 2.) and the sets of images
    Rows joined(T.q);
    std::set<uint32_t> vars, rows, slots;
    for (size_t p = 0; p < np; p++) {
        const Source &S = kSources[spec[p].src];
        for (uint32_t k = 0; k < spec[p].count; k++) {
            for (uint32_t r = 0; r < S.rows.size(); r++)
                for (const Term &t : S.rows[r]) {
                    uint32_t var, coef, row;
                    join_map(parts.data(), (uint32_t)p, k, t.var, t.coef, r, var, coef, row);
                    if (row >= T.q) return fail("row outside the totals");
                    if (coef >= ncoef) return fail("coefficient outside the totals");
                    if ((t.coef >= S.shared) != (coef >= T.shared)) return fail("a slot among the shared coefficients, or the other way round");
                    const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
                    if (kind != t.var >> 29 || (kind <= 2 && idx >= T.n) || (kind == 3 && idx >= T.m)) return fail("variable outside the totals");
                    joined[row].push_back({var, coef});
                }
            // every variable, row and slot of the copy once: images of different (part, copy, index) never meet
            for (uint32_t kind = 0; kind <= 3; kind++)
                for (uint32_t i = 0; i < (kind == 3 ? S.m : S.n); i++) {
                    uint32_t var, coef, row;
                    join_map(parts.data(), (uint32_t)p, k, V(kind, i), 0, 0, var, coef, row);
                    if (!vars.insert(var).second) return fail("two variables on one");
                }
            for (uint32_t r = 0; r < S.rows.size(); r++) {
                uint32_t var, coef, row;
                join_map(parts.data(), (uint32_t)p, k, V(4, 0), 0, r, var, coef, row);
                if (var != V(4, 0)) return fail("the constant One moved");
                if (!rows.insert(row).second) return fail("two rows on one");
            }
            for (uint32_t s = 0; s < S.n_params; s++) {
                uint32_t var, coef, row;
                join_map(parts.data(), (uint32_t)p, k, V(4, 0), S.shared + s, 0, var, coef, row);
                if (!slots.insert(coef).second) return fail("two parameter slots on one");
            }
        }
    }
    if (vars.size() != 3 * T.n + T.m || rows.size() != T.q || slots.size() != T.n_params) return fail("the map misses part of the totals");
    if (!slots.empty() && (*slots.begin() != T.shared || *slots.rbegin() != ncoef - 1)) return fail("the slots are not one range behind the shared coefficients");
    std::vector<uint64_t> wcp; std::vector<uint32_t> wer, wec;
    transpose(joined, (uint32_t)T.n, (uint32_t)T.m, wcp, wer, wec);
    if (wer.size() != T.nnz) return fail("nnz of the join");
    // 2. the replication on columns, as the kernels do it, into exact-size heap buffers
    std::vector<uint64_t> out((size_t)3 * T.n + T.m + 2, ~0ull);
    std::vector<uint32_t> orow(T.nnz, ~0u), ocoef(T.nnz, ~0u), osrc(ncoef, ~0u);
    for (size_t p = 0; p < np; p++) {
        const JoinPart &P = parts[p];
        const uint32_t ncol = 3 * P.n + P.m;
        for (uint32_t k = 0; k < P.count; k++) {
            for (uint32_t c = 0; c <= ncol; c++) {
                if (c == ncol) { if (p == 0 && k == 0) { out.at(3 * T.n + T.m) = P.sec_base[4]; out.at(3 * T.n + T.m + 1) = T.nnz; } continue; }
                const uint32_t sec = c < 3 * P.n ? c / P.n : 3u;
                uint32_t var, coef, row;
                join_map(parts.data(), (uint32_t)p, k, repeat_var_of(c, P.n, P.m), 0, 0, var, coef, row);
                uint64_t &slot = out.at(repeat_col_of(var, (uint32_t)T.n, (uint32_t)T.m));
                if (slot != ~0ull) return fail("two columns on one");
                slot = join_entry_pos(P, sec, k, cps[p][c]);
            }
            for (uint64_t e = 0; e < P.sec[5]; e++) {
                uint32_t var, coef, row;
                join_map(parts.data(), (uint32_t)p, k, 4u << 29, ecs[p][e], ers[p][e], var, coef, row);
                const uint64_t pos = join_entry_pos(P, join_section_of(P, e), k, e);
                if (pos >= T.nnz) return fail("entry position outside [0, nnz')");
                if (orow[pos] != ~0u) return fail("two entries at one position");
                orow[pos] = row; ocoef[pos] = coef;
            }
        }
        for (uint64_t i = 0; i < (uint64_t)P.shared + (uint64_t)P.count * P.n_params; i++) {       // k_join_coef: where each joined coefficient comes from
            uint32_t &dst = osrc.at(i < P.shared ? P.base_shared + i : P.base_slot + (i - P.shared));
            if (dst != ~0u) return fail("two coefficients on one");
            dst = (uint32_t)(i < P.shared ? i : P.shared + (i - P.shared) % P.n_params);
        }
    }
    for (uint32_t r : orow) if (r == ~0u) return fail("an entry position was never written");
    for (uint32_t c : osrc) if (c == ~0u) return fail("a coefficient was never written");
    for (size_t c = 0; c + 1 < out.size(); c++) if (out[c] > out[c + 1]) return fail("column pointers are not monotone");
    if (out != wcp) return fail("col_ptr of the join");
    for (size_t c = 0; c + 1 < out.size(); c++) {
        std::vector<std::pair<uint32_t, uint32_t>> a, w;
        for (uint64_t e = out[c]; e < out[c + 1]; e++) { a.push_back({orow[e], ocoef[e]}); w.push_back({wer[e], wec[e]}); }
        if (c + 2 == out.size() && !std::is_sorted(a.begin(), a.end(), [](auto &x, auto &y) { return x.first < y.first; })) return fail("the constants column is not in row order");
        std::sort(a.begin(), a.end()); std::sort(w.begin(), w.end());
        if (a != w) return fail("entries of a column");
    }
    // 3. one part: the repeat's map, term for term
    if (np == 1) {
        const Source &S = kSources[spec[0].src];
        const JoinPart &P = parts[0];
        const RepeatDims D{S.n, S.m, (uint32_t)S.rows.size(), S.shared, S.n_params};
        for (uint32_t k = 0; k < P.count; k++) {
            for (uint32_t r = 0; r < S.rows.size(); r++)
                for (const Term &t : S.rows[r]) {
                    uint32_t a[3], b[3];
                    join_map(parts.data(), 0, k, t.var, t.coef, r, a[0], a[1], a[2]);
                    repeat_map(D, k, t.var, t.coef, r, b[0], b[1], b[2]);
                    if (std::memcmp(a, b, sizeof a)) return fail("a join of one part differs from repeat_map");
                }
            for (uint64_t e = 0; e < P.sec[5]; e++) {
                const uint32_t s = join_section_of(P, e);
                if (join_entry_pos(P, s, k, e) != repeat_entry_pos(P.count, k, P.sec[s], P.sec[s + 1], e)) return fail("a join of one part differs from repeat_entry_pos");
            }
        }
    }
    return 0;
}

static scm small(uint32_t x) { uint32_t w[8] = {x, 0, 0, 0, 0, 0, 0, 0}; return sc_from_words(w); }
static uint64_t low64(const scm &s) { uint32_t w[8]; sc_to_words(w, s); for (int i = 2; i < 8; i++) if (w[i]) return ~0ull; return (uint64_t)w[1] << 32 | w[0]; }

static int check_interpreter() {
    // part 0 (67 items): n = 2, m = 1: a0 = (v0 + c0) * v0; a1 = o0 * (l0 - 1), c0 = 3 its ONE shared coefficient.
    // part 1 (3 items):  n = 3, m = 2, one checkpoint (the output of multiplier 0): a0 = (v0 + c0) * (v0 + c0) with c0 = 5 (ITS coefficient 0);
    //                    a1, a2 = bits 0 and 5 of (checkpoint + v1), level 1 (it reads the checkpoint, never a_O).
    auto cw = [](uint32_t cls, uint32_t idx) { return cls << WIT_CLASS_SHIFT | idx; };
    const std::vector<uint32_t> stream0 = {
        /* mul 0 */ 2, 1, V(3, 0), cw(WIT_COEF_PLUS_ONE, 0), V(4, 0), cw(WIT_COEF_GENERAL, 0), V(3, 0), cw(WIT_COEF_PLUS_ONE, 0),
        /* mul 1 */ 1, 2, V(2, 0), cw(WIT_COEF_PLUS_ONE, 0), V(0, 0), cw(WIT_COEF_PLUS_ONE, 0), V(4, 0), cw(WIT_COEF_MINUS_ONE, 0),
    };
    const std::vector<uint32_t> stream1 = {
        /* mul 0 */ 2, WIT_SAME_AS_LEFT, V(3, 0), cw(WIT_COEF_PLUS_ONE, 0), V(4, 0), cw(WIT_COEF_GENERAL, 0),
        /* mul 1 */ 2, WIT_HINT_BIT_PAIR | 0, V(WIT_KIND_CHECKPOINT, 0), cw(WIT_COEF_PLUS_ONE, 0), V(3, 1), cw(WIT_COEF_PLUS_ONE, 0),
        /* mul 2 */ 0, WIT_HINT_BIT_PAIR | WIT_HINT_SAME_SOURCE | 5,
    };
    std::vector<uint32_t> stream = stream0;
    stream.insert(stream.end(), stream1.begin(), stream1.end());
    JoinPart parts[2];
    std::memset(parts, 0, sizeof parts);
    parts[0].n = 2; parts[0].m = 1; parts[0].q = 1; parts[0].shared = 1; parts[0].count = 67;
    parts[1].n = 3; parts[1].m = 2; parts[1].q = 1; parts[1].shared = 1; parts[1].n_ck = 1; parts[1].count = 3;
    parts[1].stream_first = (uint32_t)stream0.size();
    const JoinTotals T = join_fill_bases(parts, 2);
    if (T.n != 143 || T.m != 73 || T.n_ck != 3 || parts[1].base_n != 134 || parts[1].base_m != 67 || parts[1].base_shared != 1) return fail("bases");
    const std::vector<scm> coef = {small(3), small(5)};
    std::vector<scm> v(T.m), ck(T.n_ck), aL(T.n), aR(T.n), aO(T.n);          // exact sizes: the last item of the last part ends at the last element
    for (uint32_t k = 0; k < 67; k++) v[k] = small(10 + k);
    for (uint32_t k = 0; k < 3; k++) { v[67 + 2 * k] = small(20 + k); v[67 + 2 * k + 1] = small(37 * k + 6); ck[k] = small((25 + k) * (25 + k)); }
    // level 0: part 0's segment and part 1's first; level 1: part 1's second.  Parts and items in reverse within a level.
    for (uint32_t k = 3; k-- > 0;) witness_eval_join_lane(parts[1], 0, 1, stream.data() + parts[1].stream_first, coef.data(), v.data(), k, aL.data(), aR.data(), aO.data(), ck.data());
    for (uint32_t k = 67; k-- > 0;) witness_eval_join_lane(parts[0], 0, 2, stream.data() + parts[0].stream_first, coef.data(), v.data(), k, aL.data(), aR.data(), aO.data(), ck.data());
    for (uint32_t k = 3; k-- > 0;) witness_eval_join_lane(parts[1], 1, 2, stream.data() + parts[1].stream_first + 6, coef.data(), v.data(), k, aL.data(), aR.data(), aO.data(), ck.data());
    for (uint32_t k = 0; k < 67; k++) {
        const uint64_t v0 = 10 + k, l0 = v0 + 3, o0 = l0 * v0;
        const uint64_t wl[2] = {l0, o0}, wr[2] = {v0, l0 - 1}, wo[2] = {o0, o0 * (l0 - 1)};
        for (uint32_t i = 0; i < 2; i++)
            if (low64(aL[2 * k + i]) != wl[i] || low64(aR[2 * k + i]) != wr[i] || low64(aO[2 * k + i]) != wo[i]) return fail("interpreter, part 0");
    }
    for (uint32_t k = 0; k < 3; k++) {
        const uint64_t l0 = 25 + k, src = l0 * l0 + 37 * k + 6;
        const uint64_t wl[3] = {l0, 1 - (src & 1), 1 - ((src >> 5) & 1)}, wr[3] = {l0, src & 1, (src >> 5) & 1}, wo[3] = {l0 * l0, 0, 0};
        for (uint32_t i = 0; i < 3; i++)
            if (low64(aL[134 + 3 * k + i]) != wl[i] || low64(aR[134 + 3 * k + i]) != wr[i] || low64(aO[134 + 3 * k + i]) != wo[i]) return fail("interpreter, part 1");
    }
    // the verify step: every flat index finds its (part, item, checkpoint), and the values hold
    for (uint64_t t = 0; t < T.n_ck; t++) {
        uint32_t p, item, c;
        join_ck_place(parts, 2, t, p, item, c);
        if (p != 1 || item != t || c != 0) return fail("join_ck_place");
        const size_t b = (size_t)parts[p].base_n + (size_t)item * parts[p].n;
        if (!witness_ck_holds(V(2, 0), ck[t], aL.data() + b, aR.data() + b, aO.data() + b)) return fail("a right checkpoint does not hold");
    }
    return 0;
}

int main() {
    const std::vector<std::vector<PartSpec>> lists = {
        {{0, 1}}, {{0, 3}}, {{1, 67}}, {{2, 2}},                   // one part: the repeat
        {{0, 2}, {1, 3}}, {{1, 3}, {0, 2}},                         // order
        {{2, 2}, {0, 1}, {1, 65}, {0, 2}, {2, 1}},                  // a template in two separate parts; a part without shared coefficients first and last
        {{1, 1}, {1, 1}, {1, 1}},
    };
    for (const auto &l : lists) if (check_matrix(l)) return 1;
    if (check_interpreter()) return 1;
    std::printf("ok\n");
    return 0;
}
