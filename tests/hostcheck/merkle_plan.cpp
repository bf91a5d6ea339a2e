// TEST HARNESS, stand-alone: replays the launch plan of a growing Merkle tree (csrc/host/merkle_plan.hpp) against brute force, and computes the
// empty-subtree constants E_0 .. E_k of a leaf with the host half of csrc/hip/k_mimc.cuh.  tests/test_merkle_grow_host.py builds it with
// -fsanitize=address,undefined and reads its output.  Usage: merkle_plan <empty leaf, 64 hex digits big-endian> <k>; prints "plan <cases> <evals>" and
// then one big-endian hex line "E <value>" for each of E_0 .. E_k.  Any broken property: a line on stderr and exit status 1.
//
// What a plan must be: the nodes it recomputes are exactly the proper ancestors of leaves [old, new), each once, bottom-up; every wide step has more than
// 256 parents; every level of the climb has at most 256; the evaluation count is the size of that set.  The climb is replayed as k_merkle_climb runs it:
// from (climb_lo, climb_hi), halving both per level, until lo reaches 1.
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_mimc.cuh"
#include "../../bulletproofs_gadgets_amd/csrc/host/merkle_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace bpg;

static const uint64_t RC[BPG_MIMC_ROUNDS][4] = {
#include "../../bulletproofs_gadgets_amd/csrc/host/mimc_rc769.inc"
};

struct Step { uint32_t level, first, count; bool wide; };

[[noreturn]] static void fail(const char *what, uint32_t depth, uint64_t old_size, uint64_t new_size) {
    std::fprintf(stderr, "merkle plan: %s at depth %u, %llu -> %llu\n", what, depth, (unsigned long long)old_size, (unsigned long long)new_size);
    std::exit(1);
}

// the plan as a list of (level, interval) in launch order, the climb's levels taken from the kernel's own loop
static std::vector<Step> replay(const MerkleGrowPlan &P, uint32_t depth, uint64_t o, uint64_t n) {
    std::vector<Step> steps;
    if (P.depth != depth || P.old_size != o || P.new_size != n) fail("the plan does not carry its input", depth, o, n);
    if (P.n_wide > MERKLE_MAX_DEPTH) fail("more wide steps than levels", depth, o, n);
    for (uint32_t k = 0; k < P.n_wide; k++) steps.push_back(Step{P.wide[k].level, P.wide[k].first, P.wide[k].count, true});
    if (!P.climb) {
        if (P.n_wide || P.evals || P.climb_evals) fail("work without a climb", depth, o, n);
        return steps;
    }
    uint32_t lo = P.climb_lo, hi = P.climb_hi, level = P.climb_level;
    if (lo < 2 || hi < lo || level < 1 || level > depth || (lo >> level) != 1 || (hi >> level) != 1) fail("the climb's entry is no interval of its level", depth, o, n);
    uint64_t climb = 0;
    do {
        lo >>= 1; hi >>= 1; level--;
        steps.push_back(Step{level, lo, hi - lo + 1, false});
        climb += hi - lo + 1;
    } while (lo > 1);
    if (level != 0 || hi != 1) fail("the climb does not end at the root", depth, o, n);
    if (climb != P.climb_evals) fail("climb_evals is not what the climb computes", depth, o, n);
    return steps;
}

// the properties that need no set: order, widths, the total
static uint64_t check_shape(const std::vector<Step> &steps, const MerkleGrowPlan &P, uint32_t depth, uint64_t o, uint64_t n) {
    uint64_t total = 0;
    for (size_t k = 0; k < steps.size(); k++) {
        const Step &s = steps[k];
        if (s.level != depth - 1 - k) fail("levels do not go bottom-up from the leaves' parents, one step each", depth, o, n);
        if (!s.count || (s.first >> s.level) != 1 || ((s.first + s.count - 1) >> s.level) != 1) fail("a step leaves its level", depth, o, n);
        if (s.wide && s.count <= MERKLE_CLIMB_PARENTS) fail("a wide step of at most 256 parents", depth, o, n);
        if (!s.wide && s.count > MERKLE_CLIMB_PARENTS) fail("a climb level of more than 256 parents", depth, o, n);
        if (k && s.wide && !steps[k - 1].wide) fail("a wide step above the climb", depth, o, n);
        total += s.count;
    }
    if (o < n && steps.size() != depth) fail("a level is missing", depth, o, n);
    if (o == n && !steps.empty()) fail("launches for no leaf", depth, o, n);
    if (total != P.evals) fail("evals is not the number of nodes the launches compute", depth, o, n);
    return total;
}

// h (of level L) is a proper ancestor of one of the leaves [o, n): its leaves are [j 2^s, (j + 1) 2^s), j = h - 2^L, s = depth - L
static bool is_ancestor(uint32_t depth, uint32_t level, uint64_t h, uint64_t o, uint64_t n) {
    const uint32_t s = depth - level;
    const uint64_t j = h - (1ull << level), a = j << s, b = (j + 1) << s;
    return a < n && o < b;
}

int main(int argc, char **argv) {
    if (argc != 3 || std::strlen(argv[1]) != 64) { std::fprintf(stderr, "usage: merkle_plan <64 hex digits, big-endian> <k>\n"); return 2; }
    uint64_t cases = 0, evals = 0;
    // every depth 1..7, every 0 <= old <= new <= 2^depth: the set itself, leaf by leaf and parent by parent
    for (uint32_t depth = 1; depth <= 7; depth++) {
        for (uint64_t o = 0; o <= (1ull << depth); o++) {
            for (uint64_t n = o; n <= (1ull << depth); n++) {
                const MerkleGrowPlan P = plan_merkle_grow(depth, o, n);
                const std::vector<Step> steps = replay(P, depth, o, n);
                evals += check_shape(steps, P, depth, o, n);
                std::vector<uint8_t> want(2ull << depth, 0), got(2ull << depth, 0);
                for (uint64_t leaf = o; leaf < n; leaf++)
                    for (uint64_t h = ((1ull << depth) + leaf) >> 1; h >= 1; h >>= 1) want[h] = 1;
                for (const Step &s : steps)
                    for (uint32_t t = 0; t < s.count; t++) if (++got.at(s.first + t) > 1) fail("a node computed twice", depth, o, n);
                if (want != got) fail("the plan's nodes are not the proper ancestors of the new leaves", depth, o, n);
                cases++;
            }
        }
    }
    // depths 20 and 24: old and new on both sides of every power of two, old = new, old = 0, new = 2^depth.  A level's ancestors are an interval (the leaves
    // are), so a step is the set when both its ends are ancestors and the nodes beside them, where the level has any, are not.
    for (uint32_t depth : {20u, 24u}) {
        std::vector<uint64_t> sizes{0};
        for (uint32_t k = 0; k <= depth; k++)
            for (int64_t d = -1; d <= 1; d++) { const int64_t v = (int64_t)(1ull << k) + d; if (v >= 0 && v <= (int64_t)(1ull << depth)) sizes.push_back((uint64_t)v); }
        for (uint64_t o : sizes) {
            for (uint64_t n : sizes) {
                if (n < o) continue;
                const MerkleGrowPlan P = plan_merkle_grow(depth, o, n);
                const std::vector<Step> steps = replay(P, depth, o, n);
                evals += check_shape(steps, P, depth, o, n);
                for (const Step &s : steps) {
                    const uint64_t a = s.first, b = (uint64_t)s.first + s.count - 1, lvl_lo = 1ull << s.level, lvl_hi = (2ull << s.level) - 1;
                    if (!is_ancestor(depth, s.level, a, o, n) || !is_ancestor(depth, s.level, b, o, n)) fail("a step computes a node that is no ancestor", depth, o, n);
                    if (a > lvl_lo && is_ancestor(depth, s.level, a - 1, o, n)) fail("an ancestor left of a step", depth, o, n);
                    if (b < lvl_hi && is_ancestor(depth, s.level, b + 1, o, n)) fail("an ancestor right of a step", depth, o, n);
                }
                cases++;
            }
        }
    }
    // what the plan refuses
    int refused = 0;
    const uint64_t bad[][3] = {{0, 0, 0}, {25, 0, 1}, {3, 5, 4}, {3, 0, 9}, {24, 0, (1ull << 24) + 1}};
    for (const auto &b : bad) { try { (void)plan_merkle_grow((uint32_t)b[0], b[1], b[2]); } catch (const std::invalid_argument &) { refused++; } }
    if (refused != 5) { std::fprintf(stderr, "merkle plan: %d of 5 bad inputs refused\n", refused); return 1; }
    std::printf("plan %llu %llu\n", (unsigned long long)cases, (unsigned long long)evals);

    // E_0 .. E_k of the given leaf
    uint8_t le[32];
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (std::sscanf(argv[1] + 2 * i, "%2x", &v) != 1) { std::fprintf(stderr, "not a hex digit\n"); return 2; }
        le[31 - i] = (uint8_t)v;
    }
    const int k = std::atoi(argv[2]);
    std::vector<scm> rc(BPG_MIMC_ROUNDS);               // on the heap: a read past the table is the sanitizer's to see
    for (int i = 0; i < BPG_MIMC_ROUNDS; i++) { uint32_t w[8]; std::memcpy(w, RC[i], 32); rc[i] = sc_from_words(w); }
    uint32_t w[8]; std::memcpy(w, le, 32);
    scm e = sc_from_words(w);
    for (int l = 0; l <= k; l++) {
        if (l) e = mimc_node(e, e, rc.data());
        sc_to_words(w, e);
        uint8_t out[32]; std::memcpy(out, w, 32);
        std::printf("E ");
        for (int i = 31; i >= 0; i--) std::printf("%02x", out[i]);
        std::printf("\n");
    }
    return 0;
}
