// MiMC Merkle trees in the prefix layout - part of kernels.cuh (included from there; see its header for the kernel map).  The layout, its invariant and the
// index rules are host/merkle_prefix_plan.hpp: height s = 0 is the leaves, s = depth the root, height s stores width[s] slots at off[s] of ONE buffer, and a
// node that is not stored has the value E[s] of the (depth + 1)-scalar table the tree owns.  Every kernel takes the dimensions as one struct by value and
// recomputes none of them.  The node function and its constants are k_mimc.cuh's: nothing here is bound by anything but its 1,944 dependent products.
#pragma once
#include "k_mimc.cuh"
#include "../host/merkle_prefix_plan.hpp"

namespace bpg {

#if defined(__HIPCC__)
// 32 bytes as they are, in two 16-byte moves
__device__ __forceinline__ void mpx_copy32(scm *dst, const scm *src) {
    const uint4 *s = reinterpret_cast<const uint4 *>(src->v);
    const uint4 a = s[0], b = s[1];
    uint4 *d = reinterpret_cast<uint4 *>(dst->v);
    d[0] = a; d[1] = b;
}
// node (s, j) wherever it lives: its slot when it is stored, the table's constant when it is not (such a node is never occupied)
__device__ __forceinline__ scm mpx_read(const scm *__restrict__ buf, const MerklePrefixDims &d, const scm *__restrict__ E, uint32_t s, uint64_t j) {
    return merkle_prefix_stored(d, s, j) ? buf[d.off[s] + (uint32_t)j] : E[s];
}
// parent (s + 1, j), j < width[s + 1], from its children at height s: the left one is stored (2j < width[s], host/merkle_prefix_plan.hpp), the two are 64
// contiguous bytes when the right one is stored too, and the right one is E[s] when 2j + 1 == width[s] - the odd-reserve edge and the spine
__device__ __forceinline__ void mpx_node(scm *buf, const MerklePrefixDims &d, const scm *__restrict__ E, uint32_t s, uint32_t j, const scm *__restrict__ rc) {
    const scm *kids = buf + d.off[s] + 2u * j;
    const scm left = kids[0], right = (2u * j + 1u < d.width[s]) ? kids[1] : E[s];
    buf[d.off[s + 1] + j] = mimc_node(left, right, rc);
}

// fill: E[s] into every stored slot that is not occupied by a tree of `size` leaves; occupied slots are left alone.  One lane per slot, two 16-byte stores.
__global__ void __launch_bounds__(256) k_mpx_fill(scm *buf, MerklePrefixDims d, uint32_t size, const scm *__restrict__ E) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= merkle_prefix_slots(d)) return;
    const uint32_t s = merkle_prefix_height_of(d, g), j = g - d.off[s];
    if (j < merkle_prefix_occupied(size, s)) return;
    mpx_copy32(buf + g, E + s);
}
// range: parents first .. first + count - 1 of height s + 1 from their children, one lane per parent (first + count <= width[s + 1])
__global__ void __launch_bounds__(256) k_mpx_range(scm *buf, MerklePrefixDims d, uint32_t s, uint32_t first, uint32_t count, const scm *__restrict__ rc, const scm *__restrict__ E) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    mpx_node(buf, d, E, s, first + t, rc);
}
// climb: from the dirty children [lo, hi] of height s (at most 256 parents above them) to the root in one launch of ONE 256-lane block.  Per level the interval
// halves and lane t <= hi - lo computes parent lo + t; a level reads what the level before wrote, so the levels are separated by a block barrier that every
// lane reaches - the loads and the store are guarded, the barrier is not.  s, lo, hi and the depth are kernel arguments, so the trip count (depth - s, up to
// 32) is uniform.  Above height ceil(lg reserve) the interval is the one node of the spine, whose right child is the table's.
__global__ void __launch_bounds__(256) k_mpx_climb(scm *buf, MerklePrefixDims d, uint32_t s, uint32_t lo, uint32_t hi, const scm *__restrict__ rc, const scm *__restrict__ E) {
    for (; s < d.depth; s++) {
        lo >>= 1; hi >>= 1;
        if (threadIdx.x <= hi - lo) mpx_node(buf, d, E, s, lo + threadIdx.x, rc);
        __syncthreads();
    }
}
// list: the node function over explicit parents (s + 1, pos[t]) of one height (the ancestors of updated leaves; distinct, so no two lanes write one node)
__global__ void __launch_bounds__(256) k_mpx_list(scm *buf, MerklePrefixDims d, uint32_t s, const uint32_t *__restrict__ pos, uint32_t count, const scm *__restrict__ rc, const scm *__restrict__ E) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    mpx_node(buf, d, E, s, pos[t], rc);
}
// set-leaves: leaf index[i] = raw[i] (32 bytes, any 256-bit value) in Montgomery form; the indices are distinct and below the tree's size, so below width[0]
__global__ void __launch_bounds__(256) k_mpx_set_leaves(scm *buf, MerklePrefixDims d, const uint32_t *__restrict__ index, const uint32_t *__restrict__ raw, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || index[i] >= d.width[0]) return;
    uint32_t w[8]; sc_load_words(w, raw + 8 * (size_t)i);
    buf[d.off[0] + index[i]] = sc_from_words(w);
}
// paths: one thread per (item, lv), lv < depth; out[item][lv] = the sibling of leaf index[item]'s ancestor at height lv, canonical bytes; ancestors != 0: the
// ancestor at height lv + 1 instead (the nodes ON the path, the root last).  Any index below 2^depth: far right of the reserve everything but the top
// siblings is the table's.  Positions are 64 bits wide and no shift reaches 32: index >> lv has lv <= 31, and the parent is one more shift by 1.
__global__ void __launch_bounds__(256) k_mpx_paths(const scm *__restrict__ buf, MerklePrefixDims d, const scm *__restrict__ E, const uint32_t *__restrict__ index, uint32_t count,
                                                   uint32_t ancestors, uint32_t *__restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;          // count * depth < 2^32 (the engine cuts longer lists into several launches)
    if (t >= count * d.depth) return;
    const uint32_t item = t / d.depth, lv = t - item * d.depth;
    const uint64_t j = (uint64_t)(index[item] >> lv);
    sc_store_canonical(out + 8 * (size_t)t, ancestors ? mpx_read(buf, d, E, lv + 1u, j >> 1) : mpx_read(buf, d, E, lv, j ^ 1ull));
}
// export: nodes first .. first + count - 1 of height s as canonical bytes (bpg_merkle_root, bpg_merkle_nodes); a position at or beyond width[s] is the table's
__global__ void __launch_bounds__(256) k_mpx_export(const scm *__restrict__ buf, MerklePrefixDims d, const scm *__restrict__ E, uint32_t s, uint64_t first, uint32_t count,
                                                    uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    sc_store_canonical(out + 8 * (size_t)i, mpx_read(buf, d, E, s, first + i));
}
// relayout: a tree of dimensions `from` into the buffer of dimensions `to` (same depth, a larger reserve: every width at least as large), one lane per NEW
// slot: the old slot's 32 bytes where the old layout stored that node, E[s] in the new slots [from.width[s], to.width[s]).  One launch.
__global__ void __launch_bounds__(256) k_mpx_relayout(scm *__restrict__ dst, MerklePrefixDims to, const scm *__restrict__ src, MerklePrefixDims from, const scm *__restrict__ E) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= merkle_prefix_slots(to)) return;
    const uint32_t s = merkle_prefix_height_of(to, g), j = g - to.off[s];
    mpx_copy32(dst + g, j < from.width[s] ? src + from.off[s] + j : E + s);
}
#endif  // __HIPCC__

}  // namespace bpg
