// The prefix layout of a resident MiMC Merkle tree (Engine::merkle_build_prefix, merkle_reserve; hip/k_merkle_prefix.cuh) and what growing such a tree
// launches, written down once: the kernels take the dimensions and the index rules from here, the engine launches from plan_merkle_prefix_grow() and
// from nothing else, and tests/hostcheck/merkle_prefix_plan.cpp replays both against brute force on the CPU.  No HIP, no allocation.
//
// A tree that only grows by append occupies a prefix of every level; everything right of the prefix is one of the depth + 1 empty-subtree constants E_s.
// So the tree stores a prefix only, and depth stops being a memory question:
//   depth D     1..32.  Height s = 0 is the leaves, s = D the root; node (s, j) has the children (s - 1, 2j) and (s - 1, 2j + 1).
//   reserve R   1 <= R <= min(2^D, 2^24): the leaves there is room for (2^24 is the bound on leaves held, so every stored position and the slot total
//               fit 32 bits).  size <= R leaves are held.
//   occupied    j < ceil(size / 2^s).  A node that is not occupied has the value E_s.
//   stored      height s keeps W_s = max(1, ceil(R / 2^s)) slots at offset off_s = sum of W_t over t < s of ONE buffer of 32-byte Montgomery scalars
//               (D = 3, R = 5: W = 5, 3, 2, 1, eleven slots; D = 32, R = 2^20: 2^21 + 11 slots, 64 MB).
//   invariant   every stored slot holds its node's value; stored slots that are not occupied hold E_s.
//   fallback    a node with j >= W_s is never stored: it is not occupied (W_s >= the occupied width), and whoever needs it reads E_s from the
//               (D + 1)-scalar table the tree owns on the device.
// An occupied parent (s + 1, j) has a stored left child (2j <= 2 ((R - 1) >> (s + 1)) <= (R - 1) >> s < W_s); its right child 2j + 1 may equal W_s when
// ceil(R / 2^s) is odd (or 1): the odd-reserve edge, and the whole one-node spine above height ceil(lg R).
//
// Growing from old_size to new_size leaves dirties positions [old_size, new_size - 1] of height 0, and dirty children [lo, hi] of any height have the
// parents [lo >> 1, hi >> 1], an interval never wider than the one below it.  The plan is
//   wide steps  one launch of k_mpx_range per height whose parent interval holds more than MERKLE_PREFIX_CLIMB_PARENTS nodes, bottom-up;
//   the climb   from the first height whose parent interval fits one block, everything up to the root in ONE launch of k_mpx_climb, entered with the
//               dirty CHILD interval of that height.  The spine is part of it.
// These are exactly the proper ancestors of the new leaves, each once; `evals` counts them.
#pragma once
#include <cstdint>
#include <stdexcept>

#if defined(__HIPCC__)
#define BPG_MPX_HD __host__ __device__ __forceinline__
#else
#define BPG_MPX_HD inline
#endif

namespace bpg {

constexpr uint32_t MERKLE_PREFIX_MAX_DEPTH = 32;
constexpr uint64_t MERKLE_PREFIX_MAX_RESERVE = 1ull << 24;
constexpr uint32_t MERKLE_PREFIX_CLIMB_PARENTS = 256;       // = BPG_MERKLE_TOP_PARENTS (hip/k_mimc.cuh): the lanes of the one block that climbs

// What every kernel of hip/k_merkle_prefix.cuh gets by value; none recomputes it.  Entries above `depth` are zero.
struct MerklePrefixDims {
    uint32_t depth, reserve;
    uint32_t off[MERKLE_PREFIX_MAX_DEPTH + 1], width[MERKLE_PREFIX_MAX_DEPTH + 1];
};

// the largest reserve a tree of this depth may have (depth 1..32)
inline uint64_t merkle_prefix_limit(uint32_t depth) { return depth >= 24 ? MERKLE_PREFIX_MAX_RESERVE : (1ull << depth); }

// Refused (std::invalid_argument, the caller's): depth outside 1..32, reserve outside 1..min(2^depth, 2^24).
inline MerklePrefixDims merkle_prefix_dims(uint32_t depth, uint64_t reserve) {
    if (depth < 1 || depth > MERKLE_PREFIX_MAX_DEPTH) throw std::invalid_argument("merkle prefix layout: depth must be 1..32");
    if (reserve < 1 || reserve > merkle_prefix_limit(depth)) throw std::invalid_argument("merkle prefix layout: reserve must be 1..min(2^depth, 2^24)");
    MerklePrefixDims d{};
    d.depth = depth; d.reserve = (uint32_t)reserve;
    uint64_t at = 0;
    for (uint32_t s = 0; s <= depth; s++) {
        const uint64_t w = (reserve + (1ull << s) - 1) >> s;        // s <= 32: a 64-bit shift
        d.width[s] = (uint32_t)(w ? w : 1);
        d.off[s] = (uint32_t)at;
        at += d.width[s];                                           // at most 2^25 + 32
    }
    return d;
}
BPG_MPX_HD uint32_t merkle_prefix_slots(const MerklePrefixDims &d) { return d.off[d.depth] + d.width[d.depth]; }
// the device bytes of a tree of these dimensions: its slots and its table of depth + 1 constants
inline uint64_t merkle_prefix_bytes(const MerklePrefixDims &d) { return 32ull * ((uint64_t)merkle_prefix_slots(d) + d.depth + 1); }

// ---- the index rules the kernels run (and the host model of the tests runs with them)
// the occupied width of height s in a tree of `size` leaves: ceil(size / 2^s), s <= 32
BPG_MPX_HD uint32_t merkle_prefix_occupied(uint32_t size, uint32_t s) { return (uint32_t)(((uint64_t)size + (1ull << s) - 1) >> s); }
// the height of stored slot g < merkle_prefix_slots(d): the offsets ascend, so the last height that starts at or before g
BPG_MPX_HD uint32_t merkle_prefix_height_of(const MerklePrefixDims &d, uint32_t g) {
    uint32_t s = 0;
    while (s < d.depth && g >= d.off[s + 1]) s++;
    return s;
}
// is node (s, j) stored?  j is 64 bits wide: a position of height 0 at depth 32 reaches 2^32 - 1, and its sibling arithmetic must not wrap
BPG_MPX_HD bool merkle_prefix_stored(const MerklePrefixDims &d, uint32_t s, uint64_t j) { return j < d.width[s]; }

// ---- the launch plan of growing
struct MerklePrefixWideStep { uint32_t height, first, count; };    // parents first .. first + count - 1 of height + 1, from their children at `height`; count > 256

struct MerklePrefixGrowPlan {
    uint32_t depth, reserve;
    uint64_t old_size, new_size;
    uint32_t n_wide;
    MerklePrefixWideStep wide[MERKLE_PREFIX_MAX_DEPTH];             // bottom-up: wide[k].height == k
    // the climb: entered with the dirty children [climb_lo, climb_hi] of height climb_height (0 <= climb_height < depth); it computes [lo >> 1, hi >> 1]
    // height by height until the root: depth - climb_height levels.  climb == false: no leaf was added, nothing is launched.
    bool climb;
    uint32_t climb_height, climb_lo, climb_hi;
    uint64_t climb_evals, evals;                                    // node evaluations of the climb, and of the whole plan
};

// Refused (std::invalid_argument, the caller's): what merkle_prefix_dims refuses, old_size > new_size, new_size > reserve (and so > 2^depth).
inline MerklePrefixGrowPlan plan_merkle_prefix_grow(uint32_t depth, uint64_t reserve, uint64_t old_size, uint64_t new_size) {
    (void)merkle_prefix_dims(depth, reserve);
    if (old_size > new_size || new_size > reserve) throw std::invalid_argument("merkle prefix plan: sizes must be old <= new <= reserve");
    MerklePrefixGrowPlan P{};
    P.depth = depth; P.reserve = (uint32_t)reserve; P.old_size = old_size; P.new_size = new_size;
    if (old_size == new_size) return P;
    uint32_t s = 0, lo = (uint32_t)old_size, hi = (uint32_t)(new_size - 1);         // < 2^24
    for (; s < depth; s++, lo >>= 1, hi >>= 1) {
        const uint32_t first = lo >> 1, count = (hi >> 1) - first + 1;
        if (count <= MERKLE_PREFIX_CLIMB_PARENTS) break;
        P.wide[P.n_wide++] = MerklePrefixWideStep{s, first, count};
        P.evals += count;
    }
    // more than 256 parents at height s + 1 need 2^(depth - s - 1) > 256, so the loop stopped at a height s <= depth - 9 < depth: the climb has a level
    P.climb = true; P.climb_height = s; P.climb_lo = lo; P.climb_hi = hi;
    for (; s < depth; s++) { lo >>= 1; hi >>= 1; P.climb_evals += hi - lo + 1; }
    P.evals += P.climb_evals;
    return P;
}

}  // namespace bpg
