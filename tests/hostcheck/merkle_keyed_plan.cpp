// TEST HARNESS, stand-alone: the keyed layout of a Merkle tree, its index rules and its hashing plan (csrc/host/merkle_keyed_plan.hpp) against brute force.
// tests/test_merkle_keyed_host.py builds it with -fsanitize=address,undefined and reads its output:
// "keyed <splits> <replacement cases> <deep cases> <evals> <merges>".  Any broken property: a line on stderr and exit status 1.
//
// The model below is the device code with the hashing taken out: a tree is, per height, an array of positions beside an array of 64-bit values, the node
// function is a 64-bit mix, and a put goes lane by lane through the SAME functions the kernels of csrc/hip/k_merkle_keyed.cuh call - classify
// (merkle_keyed_is_new), head flags (merkle_keyed_head) with an exclusive scan, the merge destinations (merkle_keyed_old_dest, _new_dest), the child lookup
// (merkle_keyed_children), find, and plan_merkle_keyed_hash.  Every access goes through at(): a read or a write outside an array ends the program here and
// would be the sanitizer's otherwise.  The arrays have a fixed capacity (16 entries and 5 heights for the small trees, 4,096 and 33 for the deep ones), so
// the 43 million small cases allocate nothing; they run on up to eight threads.
// What is checked:
//   positions stay sorted and distinct, and height s holds exactly the distinct key >> s;
//   every old value survives a merge at its new place, every destination is written exactly once;
//   the dirty lists are exactly the proper ancestors of the put keys; a brand-new parent has only brand-new dirty children;
//   the plan has wide steps only above 256 parents, bottom-up, and one climb; `evals` is the number of proper ancestors;
//   after every put EVERY node reads as brute force says: the full tree over the 2^depth-entry list at depths 1..4 - every subset of the keys with every split
//   into "held before" and "put now" (3^(2^depth) splits), and at depths 1..3 every pair of subsets (the overlap is replaced) - and a sparse tree recomputed
//   from scratch at depths 12, 31 and 32 with the keys 0, 1, 2^(depth-1) - 1, 2^(depth-1), 2^depth - 2, 2^depth - 1 and seeded random ones.
#include "../../bulletproofs_gadgets_amd/csrc/host/merkle_keyed_plan.hpp"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <thread>
#include <vector>
using namespace bpg;

[[noreturn]] static void fail(const char *what, uint32_t depth, uint64_t a, uint64_t b) {
    std::fprintf(stderr, "merkle keyed: %s at depth %u (%llu, %llu)\n", what, depth, (unsigned long long)a, (unsigned long long)b);
    std::_Exit(1);
}

static uint64_t mix(uint64_t l, uint64_t r) {                       // stands for mimc_node: any function of both children
    uint64_t x = l * 0x9e3779b97f4a7c15ull + (r ^ 0xc2b2ae3d27d4eb4full);
    x ^= x >> 29; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 32;
    return x + 0x165667b19e3779f9ull * r;
}
static const uint64_t EMPTY = 3, POISON = 0xdeadbeefdeadbeefull;
static uint64_t leaf_value(uint64_t key, uint32_t round) { return 0x1000 + 7 * key + 1000003ull * round; }
static std::atomic<uint64_t> g_evals{0}, g_merges{0};

// a vector of fixed capacity: no allocation, every access checked
template <class T, uint32_t CAP> struct Vec {
    T a[CAP]; uint32_t n = 0;
    uint32_t size() const { return n; }
    bool empty() const { return !n; }
    const T *data() const { return a; }
    T &at(uint32_t i) { if (i >= n) fail("an access outside an array", 0, i, n); return a[i]; }
    const T &at(uint32_t i) const { if (i >= n) fail("an access outside an array", 0, i, n); return a[i]; }
    void assign(uint32_t count, T v) { if (count > CAP) fail("an array beyond its capacity", 0, count, CAP); n = count; for (uint32_t i = 0; i < count; i++) a[i] = v; }
    void push_back(T v) { if (n >= CAP) fail("an array beyond its capacity", 0, n, CAP); a[n++] = v; }
    void copy(const Vec &o) { n = o.n; for (uint32_t i = 0; i < n; i++) a[i] = o.a[i]; }
};

// what a put works in: the dirty lists and brand-new positions of every height, the flags, a merge's destination
template <uint32_t CAP, uint32_t H> struct Work {
    Vec<uint32_t, CAP> dirty[H], fresh[H], fx, fy, dpos, hits;
    Vec<uint64_t, CAP> dval;
    uint64_t evals = 0, merges = 0;
};

template <uint32_t CAP, uint32_t H> struct Tree {
    uint32_t depth;
    Vec<uint32_t, CAP> pos[H];
    Vec<uint64_t, CAP> val[H];
    uint64_t E[H];
    explicit Tree(uint32_t d) : depth(d) {
        if (d + 1 > H) fail("a tree beyond its heights", d, H, 0);
        E[0] = EMPTY;
        for (uint32_t s = 0; s < d; s++) E[s + 1] = mix(E[s], E[s]);
    }
    uint64_t read(uint32_t s, uint64_t p) const {                   // mkx_read
        const uint32_t r = merkle_keyed_find(pos[s].data(), pos[s].size(), p);
        return r != MERKLE_KEYED_ABSENT ? val[s].at(r) : E[s];
    }
    // the put of the engine: keys sorted and distinct, the leaves in their order
    void put(const Vec<uint32_t, CAP> &keys, const Vec<uint64_t, CAP> &leaves, Work<CAP, H> &W) {
        const uint32_t D = depth;
        if (keys.empty()) return;
        // ---- the structure, read-only: classify, scan, scatter per height
        for (uint32_t s = 0; s <= D; s++) { W.dirty[s].n = 0; W.fresh[s].n = 0; }
        W.dirty[0].copy(keys);
        bool classify = true;
        for (uint32_t s = 0; s < D; s++) {
            const Vec<uint32_t, CAP> &d = W.dirty[s];
            const uint32_t m = d.size(), cnt = pos[s].size();
            W.fx.assign(m, 0); W.fy.assign(m, 0);
            for (uint32_t i = 0; i < m; i++) {                      // k_mkx_classify
                W.fx.at(i) = classify && merkle_keyed_is_new(pos[s].data(), cnt, d.at(i));
                W.fy.at(i) = merkle_keyed_head(d.data(), i);
            }
            uint32_t ax = 0, ay = 0;                                // the totals of the scan
            for (uint32_t i = 0; i < m; i++) { ax += W.fx.at(i); ay += W.fy.at(i); }
            W.fresh[s].assign(ax, 0xffffffffu); W.dirty[s + 1].assign(ay, 0xffffffffu);
            ax = ay = 0;
            for (uint32_t i = 0; i < m; i++) {                      // k_mkx_scatter: the exclusive ranks
                if (W.fx.at(i)) W.fresh[s].at(ax) = d.at(i);
                if (W.fy.at(i)) W.dirty[s + 1].at(ay) = d.at(i) >> 1;
                ax += W.fx.at(i); ay += W.fy.at(i);
            }
            // the dirty list above is exactly unique(p >> 1): ascending, distinct, and every parent in it
            const Vec<uint32_t, CAP> &up = W.dirty[s + 1];
            for (uint32_t i = 1; i < up.size(); i++) if (up.at(i - 1) >= up.at(i)) fail("a dirty list that is not ascending and distinct", D, s, i);
            for (uint32_t i = 0; i < m; i++) if (merkle_keyed_find(up.data(), up.size(), d.at(i) >> 1) == MERKLE_KEYED_ABSENT) fail("a parent missing from the dirty list", D, s, i);
            for (uint32_t i = 0; i < up.size(); i++)
                if (merkle_keyed_find(d.data(), m, merkle_keyed_left(up.at(i))) == MERKLE_KEYED_ABSENT && merkle_keyed_find(d.data(), m, merkle_keyed_right(up.at(i))) == MERKLE_KEYED_ABSENT)
                    fail("a dirty parent without a dirty child", D, s, i);
            // a brand-new parent has only brand-new dirty children: once a height has no brand-new position, none above has
            if (!classify) for (uint32_t i = 0; i < m; i++) if (merkle_keyed_is_new(pos[s].data(), cnt, d.at(i))) fail("a brand-new position above a height without one", D, s, i);
            if (W.fresh[s].empty()) classify = false;
        }
        if (classify && pos[D].empty()) W.fresh[D].assign(1, 0);
        if (W.dirty[D].size() != 1 || W.dirty[D].at(0) != 0) fail("the root's dirty list", D, W.dirty[D].size(), 0);
        // ---- the plan
        uint32_t counts[MERKLE_KEYED_MAX_DEPTH + 1] = {0};
        uint64_t ancestors = 0;
        for (uint32_t s = 0; s <= D; s++) { counts[s] = W.dirty[s].size(); if (s) ancestors += counts[s]; }
        const MerkleKeyedHashPlan P = plan_merkle_keyed_hash(D, counts);
        if (!P.climb || P.evals != ancestors || P.climb_height >= D) fail("the plan's climb or evals", D, P.evals, ancestors);
        for (uint32_t k = 0; k < P.n_wide; k++)
            if (P.wide[k].height != k || P.wide[k].count != counts[k + 1] || P.wide[k].count <= MERKLE_KEYED_CLIMB_PARENTS) fail("a wide step", D, k, P.wide[k].count);
        if (P.climb_height != P.n_wide) fail("the climb does not start where the wide steps end", D, P.climb_height, P.n_wide);
        for (uint32_t s = P.climb_height; s < D; s++) if (counts[s + 1] > MERKLE_KEYED_CLIMB_PARENTS) fail("a climb height wider than one block", D, s, counts[s + 1]);
        // ---- the merges: one lane per old entry, one per brand-new entry (k_mkx_merge)
        for (uint32_t s = 0; s <= D; s++) {
            const Vec<uint32_t, CAP> &fresh = W.fresh[s];
            if (fresh.empty()) continue;
            W.merges++;
            const uint32_t cnt = pos[s].size(), n_new = fresh.size(), total = cnt + n_new;
            W.dpos.assign(total, 0xffffffffu); W.hits.assign(total, 0); W.dval.assign(total, POISON);
            for (uint32_t t = 0; t < total; t++) {
                if (t < cnt) {
                    const uint32_t at = merkle_keyed_old_dest(t, pos[s].at(t), fresh.data(), n_new);
                    W.dpos.at(at) = pos[s].at(t); W.dval.at(at) = val[s].at(t); W.hits.at(at)++;
                } else {
                    const uint32_t k = t - cnt, at = merkle_keyed_new_dest(k, fresh.at(k), pos[s].data(), cnt);
                    W.dpos.at(at) = fresh.at(k); W.dval.at(at) = E[s]; W.hits.at(at)++;
                }
            }
            for (uint32_t t = 0; t < total; t++) if (W.hits.at(t) != 1) fail("a merge destination not written exactly once", D, s, t);
            for (uint32_t t = 1; t < total; t++) if (W.dpos.at(t - 1) >= W.dpos.at(t)) fail("positions not sorted and distinct after a merge", D, s, t);
            for (uint32_t t = 0; t < cnt; t++) {                    // every old value survives at its new place
                const uint32_t r = merkle_keyed_find(W.dpos.data(), total, pos[s].at(t));
                if (r == MERKLE_KEYED_ABSENT || W.dval.at(r) != val[s].at(t)) fail("an old value lost in a merge", D, s, t);
            }
            pos[s].copy(W.dpos); val[s].copy(W.dval);
        }
        // ---- the hashing: the leaves, then every dirty parent by child lookup (mkx_node), bottom-up
        for (uint32_t i = 0; i < keys.size(); i++) {
            const uint32_t at = merkle_keyed_find(pos[0].data(), pos[0].size(), keys.at(i));
            if (at == MERKLE_KEYED_ABSENT) fail("a put key that the structure did not store", D, keys.at(i), 0);
            val[0].at(at) = leaves.at(i);
        }
        for (uint32_t s = 0; s < D; s++)
            for (uint32_t i = 0; i < W.dirty[s + 1].size(); i++) {
                const uint32_t p = W.dirty[s + 1].at(i);
                uint32_t li, ri;
                merkle_keyed_children(pos[s].data(), pos[s].size(), p, &li, &ri);
                if (li == MERKLE_KEYED_ABSENT && ri == MERKLE_KEYED_ABSENT) fail("a dirty parent without a stored child", D, s, p);
                if (li != MERKLE_KEYED_ABSENT && (uint64_t)pos[s].at(li) != merkle_keyed_left(p)) fail("the left child's lookup", D, s, p);
                if (ri != MERKLE_KEYED_ABSENT && (uint64_t)pos[s].at(ri) != merkle_keyed_right(p)) fail("the right child's lookup", D, s, p);
                const uint32_t at = merkle_keyed_find(pos[s + 1].data(), pos[s + 1].size(), p);
                if (at == MERKLE_KEYED_ABSENT) fail("a dirty parent that the structure did not store", D, s, p);
                const uint64_t l = li != MERKLE_KEYED_ABSENT ? val[s].at(li) : E[s], r = ri != MERKLE_KEYED_ABSENT ? val[s].at(ri) : E[s];
                if (l == POISON || r == POISON) fail("a child read before anything wrote it", D, s, p);
                val[s + 1].at(at) = mix(l, r);
                W.evals++;
            }
    }
};

// ---------------------------------------------------------------------------------------------------- depths 1..4: the full tree, level by level
typedef Tree<16, 5> SmallTree;
typedef Work<16, 5> SmallWork;

// every node of the tree, stored or not, against the full tree over leaf[0 .. 2^depth); the stored positions of height s are those with a held key below
static void check_full(const SmallTree &t, const uint64_t *leaf, uint32_t held_mask) {
    const uint32_t n = 1u << t.depth;
    uint64_t level[16];
    uint32_t below[16];                                             // below[p] != 0: node (s, p) has a held key below it
    for (uint32_t k = 0; k < n; k++) { level[k] = leaf[k]; below[k] = held_mask >> k & 1; }
    for (uint32_t s = 0, w = n;; s++, w >>= 1) {
        uint32_t stored = 0;
        for (uint32_t p = 0; p < w; p++) {
            if (t.read(s, p) != level[p]) fail("a node that differs from brute force", t.depth, s, p);
            if (below[p]) { if (stored >= t.pos[s].size() || t.pos[s].at(stored) != p) fail("a height's positions", t.depth, s, p); stored++; }
        }
        if (stored != t.pos[s].size() || t.val[s].size() != stored) fail("a height's count", t.depth, s, stored);
        if (w == 1) break;
        for (uint32_t p = 0; p < w / 2; p++) { level[p] = mix(level[2 * p], level[2 * p + 1]); below[p] = below[2 * p] | below[2 * p + 1]; }
    }
}
static void keys_of(uint32_t mask, uint32_t n, uint32_t round, Vec<uint32_t, 16> &keys, Vec<uint64_t, 16> &leaves, uint64_t *leaf) {
    keys.n = 0; leaves.n = 0;
    for (uint32_t k = 0; k < n; k++) if (mask >> k & 1) { keys.push_back(k); leaves.push_back(leaf_value(k, round)); leaf[k] = leaves.a[leaves.n - 1]; }
}
// the `before` masks that `next` hands out: with each, every `now` disjoint from it (splits), and at depths 1..3 every `now` at all (replacements)
static void small_range(uint32_t depth, std::atomic<uint32_t> *next, std::atomic<uint64_t> *splits, std::atomic<uint64_t> *replaced) {
    const uint32_t n = 1u << depth, all = (n == 32 ? 0xffffffffu : (1u << n) - 1u);
    std::unique_ptr<SmallWork> W(new SmallWork());
    Vec<uint32_t, 16> keys; Vec<uint64_t, 16> leaves;
    uint64_t n_splits = 0, n_replaced = 0;
    for (uint32_t before = next->fetch_add(1); before <= all; before = next->fetch_add(1)) {
        uint64_t leaf0[16];
        for (uint32_t k = 0; k < n; k++) leaf0[k] = EMPTY;
        SmallTree base(depth);
        keys_of(before, n, 0, keys, leaves, leaf0);
        base.put(keys, leaves, *W);
        check_full(base, leaf0, before);
        const uint32_t rest = all & ~before;
        for (uint32_t now = rest;; now = (now - 1) & rest) {        // every subset of the rest, the empty one last
            SmallTree t = base;
            uint64_t leaf[16];
            for (uint32_t k = 0; k < n; k++) leaf[k] = leaf0[k];
            keys_of(now, n, 0, keys, leaves, leaf);
            t.put(keys, leaves, *W);
            check_full(t, leaf, before | now);
            n_splits++;
            if (!now) break;
        }
        if (depth > 3) continue;
        for (uint32_t now = 0; now <= all; now++) {                 // any subset: the overlap is replaced by other leaves
            if (!(now & before)) continue;
            SmallTree t = base;
            uint64_t leaf[16];
            for (uint32_t k = 0; k < n; k++) leaf[k] = leaf0[k];
            keys_of(now, n, 1, keys, leaves, leaf);
            t.put(keys, leaves, *W);
            check_full(t, leaf, before | now);
            n_replaced++;
        }
    }
    *splits += n_splits; *replaced += n_replaced;
    g_evals += W->evals; g_merges += W->merges;
}

// ---------------------------------------------------------------------------------------------------- depths 12, 31, 32: a sparse tree recomputed from scratch
typedef Tree<4096, 33> DeepTree;
typedef Work<4096, 33> DeepWork;

static void check_sparse(const DeepTree &t, const std::map<uint64_t, uint64_t> &held) {
    std::vector<std::map<uint64_t, uint64_t>> h(t.depth + 1);
    h[0] = held;
    for (uint32_t s = 0; s < t.depth; s++)
        for (auto &kv : h[s]) {
            const uint64_t p = kv.first >> 1;
            if (h[s + 1].count(p)) continue;
            auto l = h[s].find(2 * p), r = h[s].find(2 * p + 1);
            h[s + 1][p] = mix(l != h[s].end() ? l->second : t.E[s], r != h[s].end() ? r->second : t.E[s]);
        }
    for (uint32_t s = 0; s <= t.depth; s++) {
        if (h[s].size() != t.pos[s].size() || t.val[s].size() != t.pos[s].size()) fail("a height's count", t.depth, s, t.pos[s].size());
        uint32_t i = 0;
        for (auto &kv : h[s]) {
            if ((uint64_t)t.pos[s].at(i) != kv.first || t.val[s].at(i) != kv.second) fail("a stored node that differs from the sparse brute force", t.depth, s, kv.first);
            i++;
            if (t.read(s, kv.first) != kv.second) fail("a node that reads other than the sparse brute force", t.depth, s, kv.first);
            const uint64_t sib = merkle_keyed_sibling(kv.first);                            // the sibling, stored or not, in 64 bits
            if (s < t.depth && t.read(s, sib) != (h[s].count(sib) ? h[s].at(sib) : t.E[s])) fail("a sibling that differs from the sparse brute force", t.depth, s, sib);
        }
    }
    if (held.empty() && t.read(t.depth, 0) != t.E[t.depth]) fail("the root of the empty tree", t.depth, 0, 0);
}

static uint64_t deep_cases() {
    uint64_t cases = 0;
    uint64_t state = 0x243f6a8885a308d3ull;
    auto rnd = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    std::unique_ptr<DeepWork> W(new DeepWork());
    std::unique_ptr<Vec<uint32_t, 4096>> keys(new Vec<uint32_t, 4096>());
    std::unique_ptr<Vec<uint64_t, 4096>> leaves(new Vec<uint64_t, 4096>());
    for (uint32_t depth : {12u, 31u, 32u}) {
        const uint64_t top = (1ull << depth) - 1;
        const std::vector<uint64_t> edge = {0, 1, top / 2, top / 2 + 1, top - 1, top};     // depth 32: 0, 1, 2^31 - 1, 2^31, 2^32 - 2, 2^32 - 1
        for (uint32_t round = 0; round < 3; round++) {
            std::unique_ptr<DeepTree> t(new DeepTree(depth));
            std::map<uint64_t, uint64_t> held;
            check_sparse(*t, held);
            // the edge keys one by one, then all at once as replacements, then random batches on both sides of 256 and of 1,024 dirty parents
            std::vector<std::vector<uint64_t>> batches;
            for (uint64_t k : edge) batches.push_back({k});
            batches.push_back(edge);
            for (uint32_t size : {1u, 7u, 300u, 600u, 1500u, 5u}) {
                std::set<uint64_t> b;
                while (b.size() < size) b.insert(rnd() & top);
                if (round == 1 && !held.empty()) { auto it = held.begin(); std::advance(it, rnd() % held.size()); b.insert(it->first); }      // one held key among them
                batches.push_back(std::vector<uint64_t>(b.begin(), b.end()));
            }
            if (round == 2) {                                                               // held keys only: nothing is merged at any height
                std::vector<uint64_t> all;
                for (auto &kv : held) all.push_back(kv.first);
                batches.push_back(all);
            }
            uint32_t serial = 0;
            for (auto &b : batches) {
                std::vector<uint64_t> sorted = b;
                std::sort(sorted.begin(), sorted.end());
                bool all_held = true;
                keys->n = 0; leaves->n = 0;
                for (uint64_t k : sorted) {
                    all_held = all_held && held.count(k);
                    keys->push_back((uint32_t)k); leaves->push_back(leaf_value(k, ++serial));
                    held[k] = leaves->a[leaves->n - 1];
                }
                const uint64_t merges = W->merges;
                t->put(*keys, *leaves, *W);
                if (all_held && W->merges != merges) fail("a merge in a put of held keys only", depth, round, b.size());
                check_sparse(*t, held);
                cases++;
            }
        }
    }
    g_evals += W->evals; g_merges += W->merges;
    return cases;
}

int main() {
    // lookups at the edges of 32 bits
    const uint32_t edge[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    if (merkle_keyed_lower_bound(edge, 6, 1ull << 32) != 6 || merkle_keyed_find(edge, 6, 0xffffffffull) != 5 || merkle_keyed_find(edge, 6, 2) != MERKLE_KEYED_ABSENT ||
        merkle_keyed_find(edge, 0, 0) != MERKLE_KEYED_ABSENT || merkle_keyed_sibling(0xffffffffull) != 0xfffffffeull || merkle_keyed_right(0x7fffffffull) != 0xffffffffull ||
        merkle_keyed_left(0xffffffffull) != 0x1fffffffeull || merkle_keyed_ancestor(0xffffffffull, 32) != 0)
        fail("a lookup at the edge of 32 bits", 32, 0, 0);
    uint32_t li, ri;
    merkle_keyed_children(edge, 6, 0x7fffffffull, &li, &ri);
    if (li != 4 || ri != 5) fail("the children of the last parent", 32, li, ri);
    merkle_keyed_children(edge, 6, 0x40000000ull, &li, &ri);
    if (li != 3 || ri != MERKLE_KEYED_ABSENT) fail("a parent with a left child only", 32, li, ri);
    merkle_keyed_children(edge, 6, 0x3fffffffull, &li, &ri);
    if (li != MERKLE_KEYED_ABSENT || ri != 2) fail("a parent with a right child only", 32, li, ri);
    // the doubling policy
    if (merkle_keyed_capacity(0, 1, 1ull << 24) != MERKLE_KEYED_MIN_CAPACITY || merkle_keyed_capacity(64, 65, 1ull << 24) != 128 || merkle_keyed_capacity(64, 64, 1ull << 24) != 64 ||
        merkle_keyed_capacity(64, 1000, 1ull << 24) != 1000 || merkle_keyed_capacity(0, 1, 1) != 1 || merkle_keyed_capacity(1, 2, 2) != 2 || merkle_keyed_limit(32, 0) != (1ull << 24) ||
        merkle_keyed_limit(32, 32) != 1 || merkle_keyed_limit(10, 3) != 128)
        fail("the capacity policy", 0, 0, 0);
    // 256 and 257 dirty parents fall on the two sides of the plan's rule
    uint32_t c256[11] = {512, 256, 128, 64, 32, 16, 8, 4, 2, 1, 1}, c257[11] = {514, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1};
    const MerkleKeyedHashPlan a = plan_merkle_keyed_hash(10, c256), b = plan_merkle_keyed_hash(10, c257);
    if (a.n_wide != 0 || a.climb_height != 0 || a.evals != 512 || b.n_wide != 1 || b.climb_height != 1 || b.wide[0].count != 257 || b.evals != 521 || b.climb_evals != 264)
        fail("256 and 257 dirty parents", 10, a.n_wide, b.n_wide);
    uint32_t none[33] = {0};
    if (plan_merkle_keyed_hash(32, none).climb || plan_merkle_keyed_hash(32, none).evals) fail("a put of no key", 32, 0, 0);

    std::atomic<uint64_t> splits{0}, replaced{0};
    const uint32_t hw = std::thread::hardware_concurrency(), workers = hw < 1 ? 1 : hw > 8 ? 8 : hw;
    for (uint32_t depth = 1; depth <= 4; depth++) {
        std::vector<std::thread> pool;
        std::atomic<uint32_t> next{0};
        for (uint32_t w = 0; w < workers; w++) pool.emplace_back(small_range, depth, &next, &splits, &replaced);
        for (std::thread &th : pool) th.join();
    }
    const uint64_t deep = deep_cases();
    std::printf("keyed %llu %llu %llu %llu %llu\n", (unsigned long long)splits.load(), (unsigned long long)replaced.load(), (unsigned long long)deep,
                (unsigned long long)g_evals.load(), (unsigned long long)g_merges.load());
    return 0;
}
