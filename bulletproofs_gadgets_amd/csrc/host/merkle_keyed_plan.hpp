// The keyed layout of a resident MiMC Merkle tree (Engine::merkle_build_keyed, merkle_put; hip/k_merkle_keyed.cuh), its index rules and what a put hashes,
// written down once: the kernels take every rule from here, the engine launches the hashing from plan_merkle_keyed_hash() and from nothing else, and
// tests/hostcheck/merkle_keyed_plan.cpp replays all of it against brute force on the CPU.  No HIP, no allocation.
//
// A tree of depth D (1..32) holds n <= 2^24 distinct keys below 2^D, one leaf per key; every other leaf holds `empty`.  Node for node it is the tree
// bpg_merkle_build would build over the 2^D-entry list that is `empty` everywhere but at the keys.
//   height s    0 = the leaves, D = the root; node (s, p) has the children (s - 1, 2p) and (s - 1, 2p + 1).  Positions are below 2^(D - s) <= 2^32, and
//               everything that doubles or flips one is done in 64 bits, so 2^32 - 1 does not wrap.
//   stored      height s stores exactly the nodes with a held key below them: the distinct values key >> s, ascending, as cnt_s positions (uint32_t) beside
//               cnt_s values (32-byte Montgomery scalars), two arrays per height.  cnt_0 = n, cnt_D = (n != 0).
//   invariant   pos_s is sorted and distinct, {p >> 1 : p in pos_s} = pos_{s+1}, and val_s[i] is the value of node (s, pos_s[i]).
//   fallback    a node that is not stored has no held key below it: it reads as E_s from the (D + 1)-scalar table the tree owns on the device.
//   capacity    a height's arrays carry slack: a height that has to hold `need` entries and has room for fewer takes merkle_keyed_capacity(cap, need) =
//               max(MERKLE_KEYED_MIN_CAPACITY, 2 cap, need), capped at 2^(D - s) by the caller.  Arrays never shrink.
//
// A put of m sorted distinct keys dirties positions d_0 = keys of height 0 and d_{s+1} = unique(d_s >> 1) above: exactly the proper ancestors of the put
// keys.  A dirty position is either held (stored already) or brand-new; a brand-new parent has only brand-new dirty children, so above the first height
// without a brand-new position nothing is merged.  Hashing computes every position of d_1 .. d_D once:
//   wide steps  one launch of k_mkx_level per height s + 1 whose dirty list holds more than MERKLE_KEYED_CLIMB_PARENTS parents, bottom-up (the lists never
//               grow on the way up, so these are the lowest heights);
//   the climb   from the first height whose dirty list fits one block, everything up to the root in ONE launch of k_mkx_climb.
#pragma once
#include <cstdint>
#include <stdexcept>

// The index rules run on the device as well: hip/k_merkle_keyed.cuh includes this header behind hip/fe.cuh, whose BPG_HD marks a function for both sides.
// A translation unit of the device compiler that has not seen BPG_HD yet must not include this header first; the host compiler needs nothing.
#if defined(BPG_HD)
#define BPG_MKX_HD BPG_HD
#elif defined(__HIPCC__)
#error "include hip/fe.cuh (BPG_HD) before host/merkle_keyed_plan.hpp in a translation unit of the device compiler"
#else
#define BPG_MKX_HD inline
#endif

namespace bpg {

constexpr uint32_t MERKLE_KEYED_MAX_DEPTH = 32;
constexpr uint64_t MERKLE_KEYED_MAX_KEYS = 1ull << 24;
constexpr uint32_t MERKLE_KEYED_CLIMB_PARENTS = 256;        // = BPG_MERKLE_TOP_PARENTS (hip/k_mimc.cuh): the lanes of the one block that climbs
constexpr uint32_t MERKLE_KEYED_MIN_CAPACITY = 64;          // entries: the smallest array a height is given
constexpr uint32_t MERKLE_KEYED_SCAN_TILE = 1024;           // flags one block of the scan kernels covers: 256 lanes, four consecutive flags each
constexpr uint32_t MERKLE_KEYED_ABSENT = 0xffffffffu;       // "not stored", where an index into a height's arrays is expected

// ---- lookup in a sorted, distinct position array
// the number of positions below p (p may be 2^32: the answer is cnt)
BPG_MKX_HD uint32_t merkle_keyed_lower_bound(const uint32_t *pos, uint32_t cnt, uint64_t p) {
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)pos[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the index of position p, or MERKLE_KEYED_ABSENT
BPG_MKX_HD uint32_t merkle_keyed_find(const uint32_t *pos, uint32_t cnt, uint64_t p) {
    const uint32_t r = merkle_keyed_lower_bound(pos, cnt, p);
    return (r < cnt && (uint64_t)pos[r] == p) ? r : MERKLE_KEYED_ABSENT;
}

// ---- children, siblings, parents
BPG_MKX_HD uint64_t merkle_keyed_left(uint64_t p) { return 2 * p; }
BPG_MKX_HD uint64_t merkle_keyed_right(uint64_t p) { return 2 * p + 1; }
BPG_MKX_HD uint64_t merkle_keyed_sibling(uint64_t p) { return p ^ 1ull; }
BPG_MKX_HD uint64_t merkle_keyed_parent(uint64_t p) { return p >> 1; }
// the ancestor of leaf `key` at height s <= 32
BPG_MKX_HD uint64_t merkle_keyed_ancestor(uint64_t key, uint32_t s) { return key >> s; }
// where the two children of parent p (of the height above) sit in the arrays of the height below; a child that is not stored is MERKLE_KEYED_ABSENT and
// reads as E of that height.  The children are neighbours in the array when both are stored.
BPG_MKX_HD void merkle_keyed_children(const uint32_t *pos, uint32_t cnt, uint64_t p, uint32_t *left, uint32_t *right) {
    const uint64_t l = merkle_keyed_left(p);
    const uint32_t r = merkle_keyed_lower_bound(pos, cnt, l);
    const bool has_l = r < cnt && (uint64_t)pos[r] == l;
    const uint32_t q = r + (has_l ? 1u : 0u);
    *left = has_l ? r : MERKLE_KEYED_ABSENT;
    *right = (q < cnt && (uint64_t)pos[q] == l + 1) ? q : MERKLE_KEYED_ABSENT;
}

// ---- classify: is dirty position p held, or brand-new?
BPG_MKX_HD bool merkle_keyed_is_new(const uint32_t *pos, uint32_t cnt, uint64_t p) { return merkle_keyed_find(pos, cnt, p) == MERKLE_KEYED_ABSENT; }

// ---- merge: `cnt` old entries and `n_new` brand-new positions (sorted, distinct, none of them held) into arrays of cnt + n_new entries
// old entry i keeps its value and moves right by the number of brand-new positions below it
BPG_MKX_HD uint32_t merkle_keyed_old_dest(uint32_t i, uint32_t p, const uint32_t *fresh, uint32_t n_new) { return i + merkle_keyed_lower_bound(fresh, n_new, p); }
// brand-new entry k (position p = fresh[k]) lands behind the old positions below it
BPG_MKX_HD uint32_t merkle_keyed_new_dest(uint32_t k, uint32_t p, const uint32_t *pos, uint32_t cnt) { return k + merkle_keyed_lower_bound(pos, cnt, p); }

// ---- the dirty list of the height above: unique(p >> 1) of a sorted list; entry i starts a new parent when it is the first or its parent differs from
// its predecessor's (a head flag); the exclusive scan of the head flags is where the parent goes
BPG_MKX_HD bool merkle_keyed_head(const uint32_t *dirty, uint32_t i) { return i == 0 || (dirty[i] >> 1) != (dirty[i - 1] >> 1); }

// ---- the doubling policy of a height's arrays (see "capacity" above); `limit` = min(2^(D - s), 2^24), the most the height can ever hold
inline uint32_t merkle_keyed_capacity(uint32_t cap, uint64_t need, uint64_t limit) {
    if (need <= cap) return cap;
    uint64_t c = 2ull * cap;
    if (c < MERKLE_KEYED_MIN_CAPACITY) c = MERKLE_KEYED_MIN_CAPACITY;
    if (c < need) c = need;
    if (c > limit) c = limit;
    return (uint32_t)(c < need ? need : c);
}
// the most height s of a depth-`depth` tree can hold
inline uint64_t merkle_keyed_limit(uint32_t depth, uint32_t s) { const uint32_t b = depth - s; return b >= 24 ? MERKLE_KEYED_MAX_KEYS : (1ull << b); }

// ---- the launch plan of the hashing
struct MerkleKeyedWideStep { uint32_t height, count; };           // the `count` > 256 dirty parents of height `height` + 1, from their children at `height`

struct MerkleKeyedHashPlan {
    uint32_t depth;
    uint32_t n_wide;
    MerkleKeyedWideStep wide[MERKLE_KEYED_MAX_DEPTH];               // bottom-up: wide[k].height == k
    // the climb: heights climb_height + 1 .. depth from the dirty lists of those heights, each at most 256 long.  climb == false: no key was put.
    bool climb;
    uint32_t climb_height;
    uint64_t climb_evals, evals;                                    // node evaluations of the climb, and of the whole plan: sum over s = 1..depth of |d_s|
};

// dirty[s] = |d_s| for s = 0..depth.  Refused (std::invalid_argument): depth outside 1..32, a list that grows on the way up or shrinks below half (rounded
// up) of the one below it, more than 2^24 keys, a root list that is not one entry when keys were put.
inline MerkleKeyedHashPlan plan_merkle_keyed_hash(uint32_t depth, const uint32_t *dirty) {
    if (depth < 1 || depth > MERKLE_KEYED_MAX_DEPTH) throw std::invalid_argument("merkle keyed plan: depth must be 1..32");
    if (dirty[0] > MERKLE_KEYED_MAX_KEYS) throw std::invalid_argument("merkle keyed plan: more than 2^24 keys");
    MerkleKeyedHashPlan P{};
    P.depth = depth;
    if (!dirty[0]) return P;
    for (uint32_t s = 0; s < depth; s++)
        if (dirty[s + 1] > dirty[s] || dirty[s + 1] < (dirty[s] + 1) / 2) throw std::invalid_argument("merkle keyed plan: a dirty list that is not unique(p >> 1) of the one below");
    if (dirty[depth] != 1) throw std::invalid_argument("merkle keyed plan: the root's dirty list is one entry");
    uint32_t s = 0;
    for (; s < depth && dirty[s + 1] > MERKLE_KEYED_CLIMB_PARENTS; s++) {
        P.wide[P.n_wide++] = MerkleKeyedWideStep{s, dirty[s + 1]};
        P.evals += dirty[s + 1];
    }
    // dirty[depth] == 1, so the loop stopped at a height s < depth: the climb has a level
    P.climb = true; P.climb_height = s;
    for (; s < depth; s++) P.climb_evals += dirty[s + 1];
    P.evals += P.climb_evals;
    return P;
}

}  // namespace bpg
