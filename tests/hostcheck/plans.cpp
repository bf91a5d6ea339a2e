// TEST HARNESS, stand-alone: the MSM planner (csrc/host/msm_plan.hpp) and the fold chooser and recoders (csrc/host/fold_plan.hpp) through the host
// compiler.  tests/test_host_logic.py builds it with -fsanitize=address,undefined and expects "ok" on the last line.
//   1. plan_msm on the shapes the prover meets (the 2^20 inner-product round alone and shared, the merged A_I with most terms skipped, small sums, the
//      empty sum): every figure of the table below, the identities that tie the plan together, and each refusal with its exception type.
//   2. choose_fold row by row: the seven rules in their order, with every knob that switches one off.
//   3. The recoders on ~1,000 pseudo-random canonical scalars, on 0, 1, l - 1 and on the chosen scalars of tests/fold_cases.py, built here by the same rules (the
//      named values; a digit of +-max every w positions for w = 3..8; scalar parts of zero, of 2^L - 1 and at their extremes for 1, 2, 4, 8 parts): the
//      digits of naf256 / wnaf256 sum back to the scalar and obey the non-adjacency rule; the bitmaps and the width-w digits per part that
//      fold_recode_naf / fold_recode_wnaf write decode to the class scalars; a step list replayed on integers mod l gives sum_t s_t x_t.  Output buffers are heap blocks of EXACTLY the sizes the formulas give: an overrun is an ASan report.
#include "../../bulletproofs_gadgets_amd/csrc/host/scalar.hpp"
#include "../../bulletproofs_gadgets_amd/csrc/host/msm_plan.hpp"
#include "../../bulletproofs_gadgets_amd/csrc/host/fold_plan.hpp"
#include <cstdio>
#include <string>
#include <vector>
using namespace bpg;

static int fail(const char *what, int row = -1) { std::printf("FAILED: %s (row %d)\n", what, row); return 1; }

// ------------------------------------------------------------------------------------------------ plan_msm
struct MsmRow {
    std::vector<uint32_t> len, msm; uint32_t nmsm, skipped; bool shared;
    uint32_t W, nb, fb, CB, tmax, ntiles, CH, nchunks; bool per_bucket, quad; uint32_t lgper, window_blocks, window_threads;
};
static int check_msm() {
    const uint32_t M = 1u << 20;
    const std::vector<MsmRow> rows = {
        {{M, M, 1, M, 1}, {0, 0, 0, 1, 1}, 2, 0, false, 17, 16384, 7, 128, 513, 770, 35, 1527926, true, true, 2, 8, 0},
        {{M, M, 1, M, 1}, {0, 0, 0, 1, 1}, 2, 0, true, 16, 32768, 7, 256, 513, 770, 64, 786433, false, false, 0, 0, 256},
        {{M, M, 1}, {0, 0, 0}, 1, 0, true, 16, 32768, 7, 256, 513, 513, 64, 524289, true, false, 0, 0, 256},
        {{1000, 1000}, {0, 0}, 1, 0, false, 37, 64, 6, 1, 1, 1, 4, 18500, true, true, 0, 1, 0},
        {{M, M, 5000, 1}, {0, 0, 0, 0}, 1, 2 * M - 7000, false, 26, 512, 7, 4, 514, 514, 4, 78007, true, true, 0, 1, 0},
        {{2 * M, 2 * M}, {0, 0}, 1, 0, false, 17, 16384, 6, 256, 1024, 1024, 31, 2300103, true, true, 1, 16, 0},
        {{}, {}, 1, 0, false, 127, 2, 1, 1, 1, 0, 4, 1, false, true, 0, 1, 0},
    };
    for (size_t r = 0; r < rows.size(); r++) {
        const MsmRow &w = rows[r];
        MsmKnobs k; k.shared = w.shared;                        // defaults: cmin 2, cmax 15, cmax_shared 16, rseg 8, lgch 0, resident 1024, window_quad on, 288 quad blocks
        const MsmRun R = plan_msm(MsmShape{(uint32_t)w.len.size(), w.len.data(), w.msm.data(), w.nmsm, w.skipped}, k);
        const MsmPlan &P = R.P;
        std::printf("msm row %zu: W %u nb %u fb %u CB %u tmax %u ntiles %u CH %u nchunks %u %s %s lgper %u blocks %u threads %u live %u\n", r, P.W, P.nb, P.fb, P.CB, P.tmax,
                    R.ntiles, R.CH, R.nchunks, R.per_bucket ? "per_bucket" : "boundary", R.quad ? "quad" : "plain", R.lgper, R.window_blocks, R.window_threads, R.live);
        if (P.nmsm != w.nmsm || P.W != w.W || P.nb != w.nb || P.fb != w.fb || P.CB != w.CB || P.tmax != w.tmax || P.lgTile != 12) return fail("window / sort figures", (int)r);
        if (R.ntiles != w.ntiles || R.CH != w.CH || R.nchunks != w.nchunks) return fail("tiles / chunks", (int)r);
        if (R.per_bucket != w.per_bucket || R.quad != w.quad || R.lgper != w.lgper || R.window_blocks != w.window_blocks || R.window_threads != w.window_threads || R.shared != w.shared)
            return fail("combine / window sums", (int)r);
        uint32_t total = 0; for (uint32_t l : w.len) total += l;
        if (P.off[0] != 0 || P.off[P.W] != 254 || P.nb != (P.CB << P.fb)) return fail("off[] / nb identities", (int)r);
        if (R.b_front != std::max(R.b_digits + R.b_e1, R.b_slots) || R.b_entries != R.b_e1) return fail("arena identities", (int)r);
        if (R.total != total || R.live != total - std::min(total, w.skipped) || P.term_start[w.nmsm] != total || R.ntiles != P.tile_start[w.nmsm]) return fail("term counts", (int)r);
        if (R.nkeys != w.nmsm * P.W * P.nb || R.Mub != (uint64_t)R.live * P.W || R.K != w.nmsm * P.W * P.CB || R.nflat != R.K * P.tmax) return fail("key counts", (int)r);
        if (R.b_e1 != (((size_t)(R.live ? R.live : 1) * P.W * 4 + 255) & ~(size_t)255) || R.b_digits != (((size_t)(total ? total : 1) * P.W * 2 + 255) & ~(size_t)255))
            return fail("entry lists are sized from the live terms, digits from all", (int)r);
        if (R.bytes_starts != (size_t)(R.nkeys + 1) * 4 || R.bytes_buckets != (size_t)R.nkeys * 128 || R.bytes_wsums != (size_t)w.nmsm * P.W * 128 || R.bytes_open_keys != (size_t)R.nchunks * 4 ||
            R.bytes_counts != (size_t)(R.nflat + 1) * 4 || R.lds_digits != (size_t)P.W * P.CB * 4 || R.bytes_wq_stage != (size_t)w.nmsm * P.W * R.window_blocks * 2 * 128)
            return fail("workspace sizes", (int)r);
        for (uint32_t j = 0; j < P.W; j++) if (P.off[j + 1] <= P.off[j] || P.off[j + 1] - P.off[j] > 16u) return fail("window widths", (int)r);
        if (r == 4 && (R.live != 12001 || R.b_e1 != (((size_t)12001 * 26 * 4 + 255) & ~(size_t)255))) return fail("skip row: live terms", (int)r);
    }
    // the refusals, each with its type
    const MsmKnobs k;
    auto shape = [](const std::vector<uint32_t> &len, const std::vector<uint32_t> &msm, uint32_t nmsm) { return MsmShape{(uint32_t)len.size(), len.data(), msm.data(), nmsm, 0}; };
    const std::vector<uint32_t> one = {5}, zero = {0}, two = {5, 5}, desc = {1, 0}, huge = {(1u << 27) + 1}, res3 = {3};
    auto logic = [&](const MsmShape &s, const MsmKnobs &kn) { try { plan_msm(s, kn); } catch (const std::invalid_argument &) { return false; } catch (const std::logic_error &) { return true; } catch (...) {} return false; };
    auto invalid = [&](const MsmShape &s, const MsmKnobs &kn) { try { plan_msm(s, kn); } catch (const std::invalid_argument &) { return true; } catch (...) {} return false; };
    if (!logic(shape(one, zero, 0), k) || !logic(shape(one, zero, 5), k)) return fail("nmsm outside 1..4 is a logic_error");
    if (!logic(shape(two, desc, 2), k) || !logic(shape(one, res3, 2), k)) return fail("segments not grouped by result are a logic_error");
    if (!invalid(shape(huge, zero, 1), k)) return fail("a segment beyond 2^27 terms is an invalid_argument");
    {   // eight segments of 2^27 terms: 2^18 tiles x 26 windows x 512 coarse bins, more (bin, tile) counters than a 31-bit index holds
        const std::vector<uint32_t> len(8, 1u << 27), msm(8, 0);
        if (!invalid(shape(len, msm, 1), k)) return fail("too many tiles is an invalid_argument");
    }
    // (the LDS, ticket-array and host-slot refusals guard figures that no shape reaches through the planner: W * CB <= 13,312 counters, W <= 127 windows)
    return 0;
}

// ------------------------------------------------------------------------------------------------ choose_fold
static int check_chooser() {
    struct Row { uint32_t Mr, nterms; bool first, original, shared, tables; FoldKernel want; };
    const bool first = true, later = false, original = true, folded = false, shared = true, alone = false, ok = true, none = false;
    auto run = [](const std::vector<Row> &rows, FoldKnobs k, const char *what) {
        for (size_t r = 0; r < rows.size(); r++) {
            const Row &w = rows[r];
            k.shared = w.shared;
            const FoldShape s{w.Mr, w.nterms, w.first, w.original};
            const FoldKernel got = choose_fold(s, k, fold_wants_tables(s, k) && w.tables);      // as the engine asks: tables only where the fold wants them
            if (got != w.want) { std::printf("%s row %zu: kernel %d, expected %d\n", what, r, (int)got, (int)w.want); return 1; }
        }
        return 0;
    };
    const FoldKnobs dflt;       // wnaf 5, split_max 65536, quad, quad_w, reg_w on
    if (run({{1u << 17, 7, first, original, alone, ok, FoldKernel::Wnaf},
             {1u << 17, 7, first, original, alone, none, FoldKernel::Reg},
             {1u << 17, 7, first, original, shared, ok, FoldKernel::Wnaf},
             {1u << 14, 7, first, original, alone, ok, FoldKernel::Quad},
             {1u << 14, 7, later, folded, alone, none, FoldKernel::QuadW},
             {32, 7, later, folded, alone, none, FoldKernel::Quad},
             {1u << 16, 7, later, folded, alone, none, FoldKernel::RegW},
             {1u << 14, 7, later, folded, shared, none, FoldKernel::RegW},
             {128, 7, later, folded, shared, none, FoldKernel::Reg},
             {1u << 10, 15, later, folded, alone, none, FoldKernel::Split},
             {1u << 10, 15, later, folded, shared, none, FoldKernel::Reg},
             {32, 31, later, folded, alone, none, FoldKernel::Mem}}, dflt, "default knobs")) return fail("chooser, default knobs");
    FoldKnobs k = dflt; k.fold_quad = false;
    if (run({{1u << 10, 7, later, folded, alone, none, FoldKernel::Split}, {1u << 10, 1, later, folded, alone, none, FoldKernel::Reg}}, k, "fold_quad = 0")) return fail("chooser, fold_quad = 0");
    k = dflt; k.fold_reg_w = false;
    if (run({{1u << 16, 7, later, folded, alone, none, FoldKernel::Reg}}, k, "fold_reg_w = 0")) return fail("chooser, fold_reg_w = 0");
    k = dflt; k.fold_wnaf = 0;
    if (fold_wants_tables(FoldShape{1u << 17, 7, first, original}, k)) return fail("fold_wnaf = 0 wants no tables");
    if (run({{1u << 17, 7, first, original, alone, ok, FoldKernel::Reg}}, k, "fold_wnaf = 0")) return fail("chooser, fold_wnaf = 0");
    // what the engine relies on: tables are asked for only on the original generators and above the split bound, whoever shares the device
    k = dflt; k.shared = true;
    if (!fold_wants_tables(FoldShape{1u << 17, 7, first, original}, k) || fold_wants_tables(FoldShape{1u << 17, 7, later, folded}, k) ||
        fold_wants_tables(FoldShape{1u << 15, 7, first, original}, k)) return fail("fold_wants_tables");
    return 0;
}

// ------------------------------------------------------------------------------------------------ recoders
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static Scalar rnd_scalar() { uint8_t b[64]; for (int i = 0; i < 8; i++) { const uint64_t x = rnd64(); std::memcpy(b + 8 * i, &x, 8); } return Scalar::from_wide(b); }
static Scalar from_int(int64_t v) { return v < 0 ? -Scalar::from_u64((uint64_t)(-v)) : Scalar::from_u64((uint64_t)v); }
// sum_k d[k] 2^k mod l, by Horner from the top
static Scalar digits_value(const int8_t d[256]) {
    const Scalar step = Scalar::from_u64(1u << 16);
    Scalar acc = Scalar::zero();
    for (int k = 240; k >= 0; k -= 16) {                // sixteen digits at a time: |sum| < 2^7 * 2^16
        int64_t v = 0;
        for (int i = 15; i >= 0; i--) v = 2 * v + d[k + i];
        acc = acc * step + from_int(v);
    }
    return acc;
}
static Scalar pow2(uint32_t e) {      // 2^e mod l, e <= 255 (a table: the checks ask for it hundreds of thousands of times)
    static std::vector<Scalar> tab;
    if (tab.empty()) { tab.push_back(Scalar::one()); const Scalar two = Scalar::from_u64(2); for (int k = 1; k < 256; k++) tab.push_back(tab.back() * two); }
    return tab.at(e);
}

struct Chosen { std::string name; Scalar s; };
static std::vector<Chosen> chosen_scalars();
static int check_digits() {
    std::vector<Scalar> cases = {Scalar::zero(), Scalar::one(), -Scalar::one()};
    for (int i = 0; i < 1000; i++) cases.push_back(rnd_scalar());
    for (const Chosen &c : chosen_scalars()) cases.push_back(c.s);
    for (size_t c = 0; c < cases.size(); c++) {
        const Scalar &s = cases[c];
        if (!s.is_canonical()) return fail("test scalar not canonical", (int)c);
        int8_t d[256];
        int32_t top = naf256(s, d);
        if (digits_value(d) != s) return fail("naf256 does not sum back", (int)c);
        int32_t seen = -1;
        for (int k = 0; k < 256; k++) {
            if (!d[k]) continue;
            if (d[k] != 1 && d[k] != -1) return fail("naf256 digit", (int)c);
            if (seen >= 0 && k - seen < 2) return fail("naf256 adjacency", (int)c);
            seen = k;
        }
        if (seen != top) return fail("naf256 top", (int)c);
        for (uint32_t w = 3; w <= 8; w++) {
            top = wnaf256(s, w, d);
            if (digits_value(d) != s) return fail("wnaf256 does not sum back", (int)c);
            seen = -1;
            for (int k = 0; k < 256; k++) {
                if (!d[k]) continue;
                if (!(d[k] & 1) || d[k] >= (1 << (w - 1)) || d[k] <= -(1 << (w - 1))) return fail("wnaf256 digit", (int)c);
                if (seen >= 0 && k - seen < (int)w) return fail("wnaf256 adjacency", (int)c);
                seen = k;
            }
            if (seen != top) return fail("wnaf256 top", (int)c);
        }
        // scalar_bits: the parts of a cut scalar put it together again
        for (uint32_t parts : {1u, 2u, 4u, 8u}) {
            const uint32_t L = (254 + parts - 1) / parts;
            Scalar acc = Scalar::zero();
            for (uint32_t p = 0; p < parts; p++) acc = acc + scalar_bits(s, p * L, L) * pow2(p * L);
            if (acc != s) return fail("scalar_bits", (int)c);
        }
    }
    return 0;
}

// the group scalars against their definition, term by term
static int check_group_scalars(const std::vector<Scalar> &us, const std::vector<Scalar> &yinv_pow2, uint64_t g_M, uint32_t g_r, const std::vector<Scalar> &sG, const std::vector<Scalar> &sH) {
    const uint32_t nterms = (1u << g_r) - 1;
    if (sG.size() != nterms || sH.size() != nterms) return fail("group scalars: count");
    for (uint32_t t = 1; t <= nterms; t++) {
        Scalar g = Scalar::one(), h = Scalar::one();
        for (uint32_t k = 1; k <= g_r; k++) {
            if (!((t >> (g_r - k)) & 1u)) continue;
            const Scalar ui = us[k - 1].invert();
            g = g * us[k - 1] * us[k - 1];
            h = h * ui * ui * yinv_pow2[ceil_log2(g_M >> k)];
        }
        if (sG[t - 1] != g || sH[t - 1] != h) return fail("group scalars: value", (int)t);
    }
    return 0;
}

// ---- chosen scalars: the named values and the width / parts patterns of tests/fold_cases.py, built here by the same rules on 320-bit signed integers
struct Wide { uint64_t v[5] = {0, 0, 0, 0, 0}; };
static void wide_add(Wide &a, int64_t d, uint32_t shift) {          // a += d * 2^shift (|d| < 2^8, shift <= 254), two's complement
    Wide t;
    const uint64_t mag = (uint64_t)(d < 0 ? -d : d);
    const uint32_t limb = shift >> 6, off = shift & 63;
    t.v[limb] = mag << off;
    if (off && limb + 1 < 5) t.v[limb + 1] = mag >> (64 - off);
    unsigned __int128 c = d < 0 ? 1 : 0;                            // a - t = a + ~t + 1
    for (int k = 0; k < 5; k++) { c += (unsigned __int128)a.v[k] + (d < 0 ? ~t.v[k] : t.v[k]); a.v[k] = (uint64_t)c; c >>= 64; }
}
static void wide_mask252(Wide &a) { a.v[3] &= 0x0fffffffffffffffull; a.v[4] = 0; }
static bool wide_is_scalar(const Wide &a, Scalar &out) {            // 0 <= a < l
    if (a.v[4]) return false;
    std::memcpy(out.w, a.v, 32);
    return out.is_canonical();
}
static Scalar wide_scalar(const Wide &a) { Scalar s; if (!wide_is_scalar(a, s)) throw std::logic_error("chosen scalar out of range"); return s; }
// sum_j pick(j) 2^(w j), a digit every w positions; the top digit (the last position not above 252) takes pick's value where that keeps 0 <= s < l, else the
// largest odd positive digit that does, else none
template <class P> static Scalar width_extreme(uint32_t w, P pick) {
    const int half = 1 << (w - 1);
    const uint32_t J = 252 / w + 1;
    Wide low;
    for (uint32_t j = 0; j + 1 < J; j++) wide_add(low, pick(j), w * j);
    std::vector<int> tops = {pick(J - 1)};
    for (int t = half - 1; t > 0; t -= 2) tops.push_back(t);
    Scalar s;
    for (int t : tops) { Wide v = low; wide_add(v, t, w * (J - 1)); if (wide_is_scalar(v, s)) return s; }
    return wide_scalar(low);
}
static int turn_digit(uint32_t j) { static const int d[8] = {1, -1, 3, -3, 5, -5, 7, -7}; return d[j % 8]; }
// kind 0 low: only the lowest piece non-zero; 1 high: only the highest, the largest l allows; 2 ones: a piece of 2^Lb - 1; 3, 4 every+ / every-: every piece
// at +max digits every w positions / at 2^Lb less those, the whole cut down to the bits below 2^252
static Scalar parts_extreme(uint32_t w, uint32_t parts, int kind) {
    const uint32_t Lb = (254 + parts - 1) / parts, shift = (parts - 1) * Lb;
    const int m = (1 << (w - 1)) - 1;
    Wide s;
    auto comb = [&](Wide &x, uint32_t at, int digit) { for (uint32_t j = 0; w * j + w - 1 <= Lb; j++) wide_add(x, digit, at + w * j); };
    if (kind == 0) { comb(s, 0, m); if (parts == 1) wide_mask252(s); }
    else if (kind == 1) {
        const Scalar top = -Scalar::one();                         // l - 1
        std::memcpy(s.v, top.w, 32);
        for (uint32_t b = 0; b < shift; b++) s.v[b >> 6] &= ~(1ull << (b & 63));
    } else if (kind == 2) { wide_add(s, 1, parts > 1 ? Lb : 252); wide_add(s, -1, 0); }
    else {
        for (uint32_t p = 0; p < parts; p++) {
            if (kind == 3) comb(s, p * Lb, m);
            else { wide_add(s, 1, p * Lb + Lb); comb(s, p * Lb, -m); }
        }
        wide_mask252(s);
    }
    return wide_scalar(s);
}
static Scalar from_hex(const char *h) {                             // big-endian hex digits
    Scalar s = Scalar::zero();
    const Scalar sixteen = Scalar::from_u64(16);
    for (; *h; h++) s = s * sixteen + Scalar::from_u64((uint64_t)(*h <= '9' ? *h - '0' : *h - 'a' + 10));
    return s;
}
static std::vector<Chosen> chosen_scalars() {
    const Scalar one = Scalar::one(), two = Scalar::from_u64(2), half = two.invert();
    std::vector<Chosen> out = {
        {"0", Scalar::zero()}, {"1", one}, {"2", two}, {"3", Scalar::from_u64(3)}, {"l-1", -one}, {"l-2", -two}, {"(l-1)/2", (-one) * half}, {"(l+1)/2", half},
        {"2^252", pow2(252)}, {"2^252+1", pow2(252) + one}, {"2^252-1", pow2(252) - one},
        {"0x0555..5", from_hex("0555555555555555555555555555555555555555555555555555555555555555")},
        {"0x0aaa..a", from_hex("0aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa")},
        {"2^31", pow2(31)}, {"2^32-1", pow2(32) - one}, {"2^32", pow2(32)}, {"2^223", pow2(223)}, {"2^224", pow2(224)}, {"7*2^200", Scalar::from_u64(7) * pow2(200)}};
    for (uint32_t w = 3; w <= 8; w++) {
        const int m = (1 << (w - 1)) - 1;
        const std::string tag = "w" + std::to_string(w);
        out.push_back({tag + "+max", width_extreme(w, [&](uint32_t) { return m; })});
        out.push_back({tag + "-max", width_extreme(w, [&](uint32_t) { return -m; })});
        out.push_back({tag + "+-", width_extreme(w, [&](uint32_t j) { return (j & 1) ? m : -m; })});
        out.push_back({tag + "-+", width_extreme(w, [&](uint32_t j) { return ((j + 1) & 1) ? m : -m; })});
        if (w == 4) out.push_back({"w4turn", width_extreme(4, turn_digit)});
        static const char *const kinds[5] = {"low", "high", "ones", "every+", "every-"};
        for (uint32_t parts : {1u, 2u, 4u, 8u}) for (int kind = 0; kind < 5; kind++)
            out.push_back({tag + " parts " + std::to_string(parts) + " " + kinds[kind], parts_extreme(w, parts, kind)});
    }
    return out;
}

// One launch's worth of scalars through the three recoders, each against integer arithmetic mod l.  all_parts: every cut (1, 2, 4, 8 pieces) under every width,
// instead of the one pair that `rounds` picks.
static int check_recoded(const std::vector<Scalar> &sG, const std::vector<Scalar> &sH, const Scalar &u_ch, uint32_t Mr, uint64_t n, bool first, int rounds, bool all_parts) {
    const uint32_t nterms = (uint32_t)sG.size();
    const Scalar cls_of[4] = {Scalar::one(), u_ch, Scalar::one(), u_ch};
    {   // plain NAF bitmaps
        std::vector<uint32_t> out(fold_naf_words(nterms));
        const FoldRecode rc = fold_recode_naf(sG, sH, u_ch, Mr, n, first, out.data());
        int32_t top = -1; double adds_fm = 0;
        for (uint32_t q = 0; q < nterms; q++) for (uint32_t cls = 0; cls < 4; cls++) {
            const uint32_t *d = out.data() + ((size_t)cls * nterms + q) * 16;
            int8_t dg[256]; int adds = 0;
            for (int k = 0; k < 256; k++) {
                const bool nz = (d[k >> 5] >> (k & 31)) & 1u, neg = (d[8 + (k >> 5)] >> (k & 31)) & 1u;
                if (neg && !nz) return fail("naf bitmaps: sign without digit", rounds);
                dg[k] = nz ? (neg ? -1 : 1) : 0; adds += nz;
                if (nz && k > top) top = k;
            }
            const Scalar want = ((cls & 1) && !first) ? Scalar::zero() : (cls < 2 ? sG[q] : sH[q]) * cls_of[cls];
            if (digits_value(dg) != want) return fail("naf bitmaps do not decode to the class scalar", rounds);
            const uint64_t nB = fold_padding_lanes(q + 1, Mr, n, first);
            adds_fm += 7.0 * adds * ((cls & 1) ? (double)nB : (double)(Mr - nB));
        }
        if (rc.top != top || rc.adds_fm != adds_fm) return fail("naf bitmaps: top / additions", rounds);
    }
    for (uint32_t w = 3; w <= 8; w++) for (uint32_t pk = 0; pk < (all_parts ? 4u : 1u); pk++) {      // width-w digits per part: every (w, parts) pair comes up in several rounds
        const uint32_t parts = 1u << (all_parts ? pk : (w + rounds) % 4);
        const uint32_t L = (254 + parts - 1) / parts, nq = nterms * parts;
        std::vector<int8_t> out(fold_wnaf_bytes(nterms, parts));
        const FoldRecode rc = fold_recode_wnaf(sG, sH, u_ch, Mr, n, first, w, parts, L, out.data());
        int32_t top = -1;
        for (uint32_t q = 0; q < nterms; q++) for (uint32_t cls = 0; cls < 4; cls++) {
            Scalar acc = Scalar::zero();
            for (uint32_t p = 0; p < parts; p++) {
                const int8_t *d = out.data() + ((size_t)cls * nq + (size_t)p * nterms + q) * 256;
                acc = acc + digits_value(d) * pow2(p * L);
                for (int k = 0; k < 256; k++) {
                    if (d[k] && k > top) top = k;
                    if (d[k] && (!(d[k] & 1) || d[k] >= (1 << (w - 1)) || d[k] <= -(1 << (w - 1)))) return fail("wnaf digits: a digit outside the tables", rounds);
                }
            }
            const Scalar want = ((cls & 1) && !first) ? Scalar::zero() : (cls < 2 ? sG[q] : sH[q]) * cls_of[cls];
            if (acc != want) return fail("wnaf digits do not decode to the class scalar", rounds);
        }
        if (rc.top != top || rc.top > (int32_t)L) return fail("wnaf digits: top", rounds);
    }
    if (nterms <= 7) {      // width-4 step lists, replayed on integers mod l: acc = sum_t s_t x_t
        std::vector<uint32_t> steps((size_t)2 * QW_MAXSTEPS);
        FoldQuadW fq;
        const FoldRecode rc = fold_recode_steps(sG, sH, Mr, steps.data(), fq);
        if (fq.Mr != Mr || fq.nterms != nterms) return fail("step lists: header", rounds);
        std::vector<Scalar> x(nterms);
        for (Scalar &v : x) v = rnd_scalar();
        double dbls = 0, adds = 0;
        for (uint32_t cls = 0; cls < 2; cls++) {
            if (fq.nsteps[cls] > QW_MAXSTEPS) return fail("step lists: count", rounds);
            Scalar acc = Scalar::zero();
            for (uint32_t i = 0; i < fq.nsteps[cls]; i++) {
                const uint32_t s = steps[cls * QW_MAXSTEPS + i], nd = s & 255u, q = (s >> 8) & 7u, mult = 2 * ((s >> 11) & 3u) + 1, neg = (s >> 13) & 1u;
                if (q >= nterms || (s >> 14)) return fail("step lists: fields", rounds);
                if (i == 0 && nd) return fail("step lists: the identity is doubled", rounds);
                acc = acc * pow2(nd);
                const Scalar add = x[q] * Scalar::from_u64(mult);
                acc = neg ? acc - add : acc + add;
                dbls += nd;
            }
            acc = acc * pow2(fq.tail[cls]); dbls += fq.tail[cls]; adds += fq.nsteps[cls];
            Scalar want = Scalar::zero();
            for (uint32_t q = 0; q < nterms; q++) want = want + (cls ? sH[q] : sG[q]) * x[q];
            if (acc != want) return fail("step lists do not replay to the sum", rounds);
        }
        if (rc.dbls_w != dbls || rc.top != (int32_t)(dbls / 2.0) - 1 || rc.adds_fm != (adds * 8.0 + nterms * 2.0 * 43.0) * Mr) return fail("step lists: bookkeeping", rounds);
    }
    return 0;
}

static int check_recoders() {
    const Scalar yinv = rnd_scalar(), u_ch = rnd_scalar();
    std::vector<Scalar> yinv_pow2(21);
    yinv_pow2[0] = yinv; for (uint32_t k = 1; k <= 20; k++) yinv_pow2[k] = yinv_pow2[k - 1] * yinv_pow2[k - 1];
    int rounds = 0;
    for (uint32_t g_r = 1; g_r <= 5; g_r++) for (int rep = 0; rep < 7; rep++, rounds++) {
        const uint64_t g_M = 1ull << (g_r + 6 + rep % 3);
        const uint32_t Mr = (uint32_t)(g_M >> g_r);
        const bool first = rep & 1;
        const uint64_t n = first ? g_M - (g_M / 3) - rep : g_M;     // padding generators in several terms of a first group
        std::vector<Scalar> us(g_r), sG, sH;
        for (Scalar &u : us) u = rnd_scalar();
        if (rep == 6) us[0] = Scalar::one();                        // a trivial challenge: short digit strings
        fold_group_scalars(us, yinv_pow2, g_M, g_r, sG, sH);
        if (check_group_scalars(us, yinv_pow2, g_M, g_r, sG, sH)) return 1;
        if (check_recoded(sG, sH, u_ch, Mr, n, first, rounds, false)) return 1;
    }
    // the chosen scalars: each in every term of one side with the next in every term of the other (1, 3 and 7 terms), seven consecutive ones term by term,
    // all zero against each - after the first group and in a first group whose padding class is the scalar itself (u_ch = 1) or a random multiple of it
    const std::vector<Chosen> chosen = chosen_scalars();
    for (size_t c = 0; c < chosen.size(); c++, rounds++) {
        const Scalar &a = chosen[c].s, &b = chosen[(c + 1) % chosen.size()].s;
        for (uint32_t nterms : {1u, 3u, 7u}) {
            const uint32_t Mr = 64;
            const uint64_t g_M = (uint64_t)Mr * (nterms + 1);
            std::vector<Scalar> sG(nterms, a), sH(nterms, b), mixed(nterms), none(nterms, Scalar::zero());
            for (uint32_t t = 0; t < nterms; t++) mixed[t] = chosen[(c + t) % chosen.size()].s;
            if (check_recoded(sG, sH, Scalar::one(), Mr, g_M, false, rounds, nterms == 7)) return 1;
            if (check_recoded(mixed, none, Scalar::one(), Mr, g_M - Mr / 2, true, rounds, false)) return 1;
            if (check_recoded(none, mixed, u_ch, Mr, g_M / 2 + 1, true, rounds, false)) return 1;
        }
    }
    // what the chosen scalars are for, read off the recoder's own output: the densest step list (64 steps per term, 448 of QW_MAXSTEPS at seven terms), a doublings
    // field of 252, a tail of 252 doublings, an empty list beside a full one
    {
        std::vector<uint32_t> steps((size_t)2 * QW_MAXSTEPS);
        FoldQuadW fq;
        const Scalar dense = width_extreme(4, [](uint32_t) { return -7; });
        const std::vector<Scalar> d7(7, dense), z7(7, Scalar::zero()), p7(7, pow2(252)), q7(7, pow2(252) + Scalar::one());
        fold_recode_steps(z7, d7, 64, steps.data(), fq);
        if (fq.nsteps[0] != 0 || fq.nsteps[1] != 448 || fq.tail[0] != 0 || fq.tail[1] != 0) return fail("step lists: empty beside densest");
        fold_recode_steps(p7, q7, 64, steps.data(), fq);
        if (fq.nsteps[0] != 7 || fq.tail[0] != 252 || fq.nsteps[1] != 14 || fq.tail[1] != 0 || (steps[QW_MAXSTEPS + 7] & 255u) != 252) return fail("step lists: 2^252 and 2^252 + 1");
    }
    // a list that cannot hold its steps is refused: 15 full-width scalars make about 15 * 51 additions per class
    {
        std::vector<Scalar> sG(31), sH(31);
        for (Scalar &s : sG) s = rnd_scalar();
        for (Scalar &s : sH) s = rnd_scalar();
        std::vector<uint32_t> steps((size_t)2 * QW_MAXSTEPS);
        FoldQuadW fq;
        bool refused = false;
        try { fold_recode_steps(sG, sH, 64, steps.data(), fq); } catch (const std::logic_error &) { refused = true; }
        if (!refused) return fail("step list overflow is a logic_error");
    }
    return 0;
}

int main() {
    static_assert(sizeof(MsmPlan) == 4 * 5 + 132 + 4 * 2 + 4 * 5 + 4 * 5 + 4 * 8, "MsmPlan is a kernel argument: its layout is fixed");
    static_assert(sizeof(FoldGroup) == 20 && sizeof(FoldWnaf) == 32 && sizeof(FoldQuadW) == 24, "the fold parameter structs are kernel arguments: their layouts are fixed");
    if (check_msm()) return 1;
    if (check_chooser()) return 1;
    if (check_digits()) return 1;
    if (check_recoders()) return 1;
    for (const Chosen &c : chosen_scalars()) {                     // printed for tests/test_plans_host.py, which compares them with tests/fold_cases.py
        uint8_t b[32]; c.s.to_bytes(b);
        std::printf("chosen [%s] ", c.name.c_str());
        for (int i = 31; i >= 0; i--) std::printf("%02x", b[i]);
        std::printf("\n");
    }
    std::printf("ok\n");
    return 0;
}
