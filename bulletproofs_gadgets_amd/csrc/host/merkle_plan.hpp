// What growing a resident MiMC Merkle tree from `old_size` to `new_size` leaves launches (Engine::merkle_build_partial with old_size = 0,
// Engine::merkle_append; hip/k_mimc.cuh), decided before anything is launched.  plan_merkle_grow() is a pure function of (depth, old size, new size) - no
// HIP, no allocation - so tests/hostcheck/merkle_plan.cpp replays it against brute force on the CPU; the engine launches from the value it returns and
// from nothing else.
//
// The tree is one heap array: the root at 1, the children of h at 2h and 2h + 1, the leaves at [2^depth, 2^(depth+1)); level L holds [2^L, 2^(L+1)).
// New leaves [old_size, new_size) dirty the heap interval [lo, hi] = [2^depth + old_size, 2^depth + new_size - 1] of the leaf level, and the dirty
// children [lo, hi] of any level have the parents [lo >> 1, hi >> 1]: an interval again, never wider than the one below it.  So the plan is
//   wide steps  one launch of k_merkle_level_range per level whose parent interval holds more than MERKLE_CLIMB_PARENTS nodes, bottom-up;
//   the climb   from the first level whose parent interval fits one block, everything up to the root in ONE launch of k_merkle_climb, entered with the
//               dirty CHILD interval of that level.
// These are exactly the proper ancestors of the new leaves, each once; `evals` counts them.
#pragma once
#include <cstdint>
#include <stdexcept>

namespace bpg {

constexpr uint32_t MERKLE_MAX_DEPTH = 24;
constexpr uint32_t MERKLE_CLIMB_PARENTS = 256;      // = BPG_MERKLE_TOP_PARENTS (hip/k_mimc.cuh): the lanes of the one block that climbs

struct MerkleWideStep { uint32_t level, first, count; };            // parents first .. first + count - 1 (heap indices) of `level`; count > MERKLE_CLIMB_PARENTS

struct MerkleGrowPlan {
    uint32_t depth;
    uint64_t old_size, new_size;
    uint32_t n_wide;
    MerkleWideStep wide[MERKLE_MAX_DEPTH];                          // bottom-up: wide[k + 1].level == wide[k].level - 1
    // the climb: entered with the dirty children [climb_lo, climb_hi] of level climb_level (1 <= climb_level <= depth, climb_lo >= 2); it computes
    // [lo >> 1, hi >> 1] level by level until the root.  climb == false: no leaf was added, nothing is launched.
    bool climb;
    uint32_t climb_level, climb_lo, climb_hi;
    uint64_t climb_evals, evals;                                    // node evaluations of the climb, and of the whole plan
};

// Refused (std::invalid_argument, the caller's): depth outside 1..24, old_size > new_size, new_size > 2^depth.
inline MerkleGrowPlan plan_merkle_grow(uint32_t depth, uint64_t old_size, uint64_t new_size) {
    if (depth < 1 || depth > MERKLE_MAX_DEPTH) throw std::invalid_argument("merkle plan: depth must be 1..24");
    if (old_size > new_size || new_size > (1ull << depth)) throw std::invalid_argument("merkle plan: sizes must be old <= new <= 2^depth");
    MerkleGrowPlan P{};
    P.depth = depth; P.old_size = old_size; P.new_size = new_size;
    if (old_size == new_size) return P;
    uint32_t level = depth;
    uint32_t lo = (uint32_t)((1ull << depth) + old_size), hi = (uint32_t)((1ull << depth) + new_size - 1);      // < 2^25
    for (; level > 0; level--, lo >>= 1, hi >>= 1) {
        const uint32_t first = lo >> 1, count = (hi >> 1) - first + 1;
        if (count <= MERKLE_CLIMB_PARENTS) break;
        P.wide[P.n_wide++] = MerkleWideStep{level - 1, first, count};
        P.evals += count;
    }
    // more than 256 parents need a level of at least 512 nodes, so the loop stopped at a level >= 9 > 0: the climb always has a level to compute
    P.climb = true; P.climb_level = level; P.climb_lo = lo; P.climb_hi = hi;
    for (; level > 0; level--) { lo >>= 1; hi >>= 1; P.climb_evals += hi - lo + 1; }
    P.evals += P.climb_evals;
    return P;
}

}  // namespace bpg
