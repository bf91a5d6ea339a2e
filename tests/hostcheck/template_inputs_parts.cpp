// TEST HARNESS, stand-alone: the branches that PUBLIC INPUTS add to the index maps of repeated and joined templates, the index arithmetic of the slot kernel
// k_input_slots_join and the two lane functions with per-item inputs (csrc/hip/k_repeat.cuh, csrc/hip/k_join.cuh: the BPG_HD half) compiled for the host.
// tests/test_template_repeat_inputs_host.py builds it with -fsanitize=address,undefined and expects "ok" on the last line.  Every buffer has EXACTLY the size
// the formulas give, so the last slot, input and multiplier of the last item of the last part is the last element.
//   1. repeat_map over [shared | K n_params | K n_slots]: shared coefficients stay, parameter and derived slots of different items never meet, each range is
//      filled exactly, and a derived slot sits at param_first + K n_params + k n_slots + s.  With n_slots = 0 the map is the old one.
//   2. join_map likewise over parts with and without inputs, the same template as two parts, a part with m = 0; k_join_coef's source index per joined slot.
//   3. join_slot_place is a bijection from [0, n_slots') onto (part, item, slot) and agrees with join_map; join_input_slot_lane writes coef[shared_p + ci] x
//      in[(p, k, input)] into exactly the derived range and nothing else.
//   4. witness_eval_repeat_lane and witness_eval_join_lane with inputs over a hand-packed program, 67 items (more than one block of 64), against plain integers.
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_join.cuh"
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
using namespace bpg;

static int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }
static uint32_t V(uint32_t kind, uint32_t idx) { return kind << 29 | idx; }
static scm small(uint64_t x) { uint32_t w[8] = {(uint32_t)x, (uint32_t)(x >> 32), 0, 0, 0, 0, 0, 0}; return sc_from_words(w); }
static uint64_t low64(const scm &s) { uint32_t w[8]; sc_to_words(w, s); for (int i = 2; i < 8; i++) if (w[i]) return ~0ull; return (uint64_t)w[1] << 32 | w[0]; }

// a template's coefficient layout and input side: [0, shared) | n_params | n_slots; pairs = (input, coefficient index) per derived slot
struct Source { uint32_t n, m, q, shared, n_params, n_in; std::vector<uint32_t> pairs; };
static const Source kSources[4] = {
    {3, 2, 4, 4, 1, 2, {0, 1, 1, 3, 0, 2}},      // all three ranges live; input 0 under two coefficients (two slots)
    {2, 1, 2, 2, 0, 0, {}},                       // no inputs at all
    {1, 0, 2, 3, 0, 3, {2, 0}},                   // m = 0, no parameter, three inputs of which the rows name one
    {5, 1, 3, 1, 2, 1, {}},                       // inputs only in multiplier operands: n_in > 0, n_slots = 0
};

static int check_repeat(const Source &S, uint32_t K) {
    const uint32_t ns = (uint32_t)S.pairs.size() / 2, ncoef = S.shared + K * (S.n_params + ns);
    const RepeatDims D{S.n, S.m, S.q, S.shared, S.n_params, ns, K}, old{S.n, S.m, S.q, S.shared, S.n_params};
    std::vector<uint8_t> hit(ncoef, 0);                       // exact size: an image outside the table is a heap overflow under ASan
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t c = 0; c < S.shared + S.n_params + ns; c++) {
            uint32_t var, coef, row;
            repeat_map(D, k, V(4, 0), c, S.q - 1, var, coef, row);
            if (var != V(4, 0) || row != k * S.q + S.q - 1) return fail("repeat_map: One or the row moved");
            if (c < S.shared) { if (coef != c) return fail("repeat_map: a shared coefficient moved"); continue; }
            if (c < S.shared + S.n_params) { if (coef != S.shared + k * S.n_params + (c - S.shared)) return fail("repeat_map: parameter slot"); }
            else if (coef != S.shared + K * S.n_params + k * ns + (c - S.shared - S.n_params)) return fail("repeat_map: derived slot");
            if (hit.at(coef)++) return fail("repeat_map: two slots on one");
            if (c < S.shared + S.n_params) {                  // without inputs: today's answers
                uint32_t a[3];
                repeat_map(old, k, V(4, 0), c, S.q - 1, a[0], a[1], a[2]);
                if (a[1] != coef) return fail("repeat_map: a parameter slot moved with the inputs");
            }
        }
    for (uint32_t c = S.shared; c < ncoef; c++) if (hit[c] != 1) return fail("repeat_map: a slot of the table is never named");
    return 0;
}

struct PartSpec { int src; uint32_t count; };

static int check_join(const std::vector<PartSpec> &spec) {
    const size_t np = spec.size();
    std::vector<JoinPart> parts(np);
    std::vector<uint32_t> pairs;
    for (size_t p = 0; p < np; p++) {
        const Source &S = kSources[spec[p].src];
        JoinPart &P = parts[p];
        std::memset(&P, 0, sizeof P);
        P.n = S.n; P.m = S.m; P.q = S.q; P.shared = S.shared; P.n_params = S.n_params; P.count = spec[p].count; P.n_in = S.n_in; P.n_slots = (uint32_t)S.pairs.size() / 2;
        pairs.insert(pairs.end(), S.pairs.begin(), S.pairs.end());
    }
    const JoinTotals T = join_fill_bases(parts.data(), np);
    const uint64_t ncoef = T.shared + T.n_params + T.n_slots;
    // 2. the map over the three ranges, and where k_join_coef takes every joined coefficient from
    std::vector<uint8_t> hit(ncoef, 0);
    std::vector<uint32_t> src(ncoef, ~0u);
    uint64_t ins = 0, pair_at = 0;
    for (size_t p = 0; p < np; p++) {
        const Source &S = kSources[spec[p].src];
        const JoinPart &P = parts[p];
        if (P.base_in != ins || P.slot_list_first != pair_at) return fail("join_fill_bases: input or pair base");
        ins += (uint64_t)P.count * P.n_in; pair_at += P.n_slots;
        for (uint32_t k = 0; k < P.count; k++)
            for (uint32_t c = 0; c < S.shared + S.n_params + P.n_slots; c++) {
                uint32_t var, coef, row;
                join_map(parts.data(), (uint32_t)p, k, V(4, 0), c, 0, var, coef, row);
                const bool shared = c < S.shared, par = !shared && c < S.shared + S.n_params;
                if (shared ? coef >= T.shared : par ? (coef < T.shared || coef >= T.shared + T.n_params) : (coef < T.shared + T.n_params || coef >= ncoef)) return fail("join_map: wrong range");
                if (shared && k) continue;                    // (every item names the part's one shared copy)
                if (hit.at(coef)++) return fail("join_map: two coefficients on one");
            }
        const uint64_t par_end = (uint64_t)P.shared + (uint64_t)P.count * P.n_params;
        for (uint64_t i = 0; i < par_end + (uint64_t)P.count * P.n_slots; i++) {
            uint32_t &dst = src.at(i < P.shared ? P.base_shared + i : i < par_end ? P.base_slot + (i - P.shared) : P.base_dslot + (i - par_end));
            if (dst != ~0u) return fail("k_join_coef: two sources for one coefficient");
            dst = (uint32_t)(i < P.shared ? i : i < par_end ? P.shared + (i - P.shared) % P.n_params : P.shared + P.n_params + (i - par_end) % P.n_slots);
            if (dst >= P.shared + P.n_params + P.n_slots) return fail("k_join_coef: source outside the part's table");
        }
    }
    if (ins != T.n_in) return fail("join_fill_bases: input total");
    for (uint64_t c = 0; c < ncoef; c++) if (hit[c] != 1 || src[c] == ~0u) return fail("join_map: a coefficient of the table is never named or never written");
    // 3. the slot kernel: place, then the lane over exact-size buffers
    std::set<uint64_t> seen;
    for (uint64_t t = 0; t < T.n_slots; t++) {
        uint32_t p, item, s;
        join_slot_place(parts.data(), (uint32_t)np, t, p, item, s);
        if (p >= np || item >= parts[p].count || s >= parts[p].n_slots) return fail("join_slot_place: outside the part");
        uint32_t var, coef, row;
        join_map(parts.data(), p, item, V(4, 0), parts[p].shared + parts[p].n_params + s, 0, var, coef, row);
        if (coef != T.shared + T.n_params + t) return fail("join_slot_place disagrees with join_map");
        if (!seen.insert((uint64_t)p << 48 | (uint64_t)item << 16 | s).second) return fail("join_slot_place: two indices on one place");
    }
    std::vector<scm> coef(ncoef), in(T.n_in);
    for (uint64_t c = 0; c < ncoef; c++) coef[c] = small(c < T.shared ? 1000 + 7 * c : 1);
    for (uint64_t i = 0; i < T.n_in; i++) in[i] = small(3 + 5 * i);
    for (uint64_t t = T.n_slots; t-- > 0;) join_input_slot_lane(parts.data(), (uint32_t)np, t, pairs.data(), in.data(), coef.data());
    for (uint64_t c = 0; c < T.shared + T.n_params; c++) if (low64(coef[c]) != (c < T.shared ? 1000 + 7 * c : 1)) return fail("the slot lane wrote outside the derived range");
    for (size_t p = 0; p < np; p++) {
        const Source &S = kSources[spec[p].src];
        const JoinPart &P = parts[p];
        for (uint32_t k = 0; k < P.count; k++)
            for (uint32_t s = 0; s < P.n_slots; s++) {
                const uint64_t want = (1000 + 7 * (uint64_t)(P.base_shared + S.pairs[2 * s + 1])) * (3 + 5 * ((uint64_t)P.base_in + (uint64_t)k * P.n_in + S.pairs[2 * s]));
                if (low64(coef[(size_t)P.base_dslot + (size_t)k * P.n_slots + s]) != want) return fail("the slot lane: wrong product");
            }
    }
    return 0;
}

static int check_lanes() {
    // n = 2, m = 1, two inputs, ONE shared coefficient c0: a0 = (v0 + x1) * (c0 x0); a1 = bit 1 of (x0 + o0) (a hint whose source names an input)
    auto cw = [](uint32_t cls, uint32_t idx) { return cls << WIT_CLASS_SHIFT | idx; };
    const std::vector<uint32_t> prog = {
        /* mul 0 */ 2, 1, V(3, 0), cw(WIT_COEF_PLUS_ONE, 0), V(WIT_KIND_INPUT, 1), cw(WIT_COEF_PLUS_ONE, 0), V(WIT_KIND_INPUT, 0), cw(WIT_COEF_GENERAL, 0),
        /* mul 1 */ 2, WIT_HINT_BIT_PAIR | 1, V(WIT_KIND_INPUT, 0), cw(WIT_COEF_PLUS_ONE, 0), V(2, 0), cw(WIT_COEF_PLUS_ONE, 0),
    };
    auto want = [](uint64_t v0, uint64_t x0, uint64_t x1, uint64_t c0, uint64_t wl[2], uint64_t wr[2], uint64_t wo[2]) {
        wl[0] = v0 + x1; wr[0] = c0 * x0; wo[0] = wl[0] * wr[0];
        const uint64_t b = ((x0 + wo[0]) >> 1) & 1;
        wl[1] = 1 - b; wr[1] = b; wo[1] = 0;
    };
    // the repeat: 67 items, item k's inputs at in + 2 k
    {
        const uint32_t K = 67;
        const std::vector<scm> coef = {small(3)};
        std::vector<scm> v(K), in(2 * K), aL(2 * K), aR(2 * K), aO(2 * K);
        for (uint32_t k = 0; k < K; k++) { v[k] = small(10 + k); in[2 * k] = small(100 + 3 * k); in[2 * k + 1] = small(7 * k); }
        for (uint32_t k = K; k-- > 0;) witness_eval_repeat_lane(0, 2, prog.data(), coef.data(), v.data(), 2, 1, k, aL.data(), aR.data(), aO.data(), nullptr, 0, in.data(), 2);
        for (uint32_t k = 0; k < K; k++) {
            uint64_t wl[2], wr[2], wo[2];
            want(10 + k, 100 + 3 * k, 7 * k, 3, wl, wr, wo);
            for (uint32_t i = 0; i < 2; i++)
                if (low64(aL[2 * k + i]) != wl[i] || low64(aR[2 * k + i]) != wr[i] || low64(aO[2 * k + i]) != wo[i]) return fail("repeat lane with inputs");
        }
    }
    // the join: (the program with inputs, 67), (a part without inputs: a0 = v0 * v0, 3), (the program with inputs again, 1)
    {
        const std::vector<uint32_t> plain = {1, WIT_SAME_AS_LEFT, V(3, 0), cw(WIT_COEF_PLUS_ONE, 0)};
        std::vector<uint32_t> stream = prog;
        stream.insert(stream.end(), plain.begin(), plain.end());
        JoinPart parts[3];
        std::memset(parts, 0, sizeof parts);
        parts[0].n = 2; parts[0].m = 1; parts[0].shared = 1; parts[0].count = 67; parts[0].n_in = 2;
        parts[1].n = 1; parts[1].m = 1; parts[1].count = 3; parts[1].stream_first = (uint32_t)prog.size();
        parts[2] = parts[0]; parts[2].count = 1;
        const JoinTotals T = join_fill_bases(parts, 3);
        if (T.n != 139 || T.m != 71 || T.n_in != 136 || T.shared != 2 || parts[2].base_in != 134 || parts[2].base_shared != 1 || parts[1].base_in != 134) return fail("bases");
        const std::vector<scm> coef = {small(3), small(11)};
        std::vector<scm> v(T.m), in(T.n_in), aL(T.n), aR(T.n), aO(T.n);
        for (uint32_t i = 0; i < T.m; i++) v[i] = small(10 + i);
        for (uint32_t i = 0; i < T.n_in; i++) in[i] = small(100 + 3 * i);
        for (uint32_t p = 3; p-- > 0;)
            for (uint32_t k = parts[p].count; k-- > 0;)
                witness_eval_join_lane(parts[p], 0, parts[p].n, stream.data() + parts[p].stream_first, coef.data(), v.data(), k, aL.data(), aR.data(), aO.data(), nullptr, in.data());
        for (uint32_t p = 0; p < 3; p += 2)
            for (uint32_t k = 0; k < parts[p].count; k++) {
                uint64_t wl[2], wr[2], wo[2];
                const uint32_t b = parts[p].base_n + 2 * k, bi = parts[p].base_in + 2 * k;
                want(10 + parts[p].base_m + k, 100 + 3 * bi, 100 + 3 * (bi + 1), p ? 11 : 3, wl, wr, wo);
                for (uint32_t i = 0; i < 2; i++)
                    if (low64(aL[b + i]) != wl[i] || low64(aR[b + i]) != wr[i] || low64(aO[b + i]) != wo[i]) return fail("join lane with inputs");
            }
        for (uint32_t k = 0; k < 3; k++) {
            const uint64_t x = 10 + 67 + k;
            if (low64(aL[134 + k]) != x || low64(aR[134 + k]) != x || low64(aO[134 + k]) != x * x) return fail("join lane of the part without inputs");
        }
    }
    return 0;
}

int main() {
    for (const Source &S : kSources) for (uint32_t K : {1u, 2u, 3u, 65u}) if (check_repeat(S, K)) return 1;
    const std::vector<std::vector<PartSpec>> lists = {
        {{0, 1}}, {{0, 3}}, {{2, 65}},                              // one part: the repeat
        {{0, 2}, {1, 3}, {0, 1}},                                   // (with inputs, 2), (without, 3), (with, 1): the same template as two parts
        {{1, 2}, {2, 3}, {3, 2}, {0, 2}},                           // a part without inputs first; m = 0; a part with inputs and no slots
        {{3, 1}, {1, 1}},                                           // no derived slot anywhere
    };
    for (const auto &l : lists) if (check_join(l)) return 1;
    if (check_lanes()) return 1;
    std::printf("ok\n");
    return 0;
}
