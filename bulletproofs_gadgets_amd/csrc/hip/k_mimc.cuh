// MiMC-x^3 over the scalar field and Merkle trees of two-block sponge nodes - part of kernels.cuh (included from there; see its header for the kernel map).
// The node function is the native form of what MerkleTree256 constrains for a (W W) node (reference src/mimc_hash/mimc.rs:7-40): two permutations of 486
// rounds, 1,944 dependent Montgomery products.  The arithmetic half of this file is BPG_HD and has no HIP in it, so tests/hostcheck compiles it for the host.
#pragma once
#include "sc.cuh"

namespace bpg {

#define BPG_MIMC_ROUNDS 486
#define BPG_MERKLE_TOP_PARENTS 256u     // levels with at most this many parents run in ONE launch of one block (k_merkle_top)
#if defined(__HIPCC__)
#define BPG_ROLLED _Pragma("unroll 1")
#else
#define BPG_ROLLED
#endif

// mimc_encryption with key 0 (host/gadgets.hpp:99-103): x, the constants and the result in Montgomery form.  The loop stays rolled: a round is ~700
// instructions, and every lane of a wave reads the same constant in the same round.
BPG_HD scm mimc_permute(scm x, const scm *rc) {
    BPG_ROLLED for (int i = 0; i < BPG_MIMC_ROUNDS; i++) {
        const scm t = sc_add(x, rc[i]);
        x = sc_mont_mul(sc_mont_mul(t, t), t);
    }
    return x;
}
// mimc_sponge_1 over (left, right): the parent of two children as they are (leaves are not hashed first)
BPG_HD scm mimc_node(const scm &left, const scm &right, const scm *rc) { return mimc_permute(sc_add(mimc_permute(left, rc), right), rc); }

#if defined(__HIPCC__)
// The constants: every lane reads the same one in the same round and the rolled loop indexes the table by its counter, so the compiler issues one scalar load per
// round and the constant sits in SGPRs.  Staging the 15,552 bytes in LDS per block was measured beside this and bought nothing, so it is gone.
__device__ __forceinline__ void sc_load_words(uint32_t w[8], const uint32_t *p) {
    const uint4 *src = reinterpret_cast<const uint4 *>(p);
    const uint4 a = src[0], b = src[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void sc_store_canonical(uint32_t *p, const scm &a) {
    uint32_t w[8]; sc_to_words(w, a);
    uint4 *dst = reinterpret_cast<uint4 *>(p);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]); dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// mimc_sponge_1 of `count` items of `blocks` 32-byte little-endian blocks each, one lane per item: state = 0; state = permute(state + block).  A block is any
// 256-bit value (taken mod l, as the host's `state += b` takes it); the output is canonical.
__global__ void __launch_bounds__(256) k_mimc_sponge(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t count, uint32_t blocks, const scm *__restrict__ rc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    scm state = sc_zero();
    BPG_ROLLED for (uint32_t b = 0; b < blocks; b++) {
        uint32_t w[8]; sc_load_words(w, in + 8 * ((size_t)i * blocks + b));
        state = mimc_permute(sc_add(state, sc_from_words(w)), rc);
    }
    sc_store_canonical(out + 8 * (size_t)i, state);
}

// The tree: ONE array of 2^(d+1) scalars in heap order - the root at 1, the children of h at 2h and 2h + 1, the leaves at [2^d, 2^(d+1)) - in Montgomery
// form throughout.  Level L holds the 2^L nodes [2^L, 2^(L+1)); d <= 24, so a heap index fits 32 bits with room to spare.
// 32-byte leaves as uploaded -> Montgomery form, in place
__global__ void __launch_bounds__(256) k_merkle_leaves(scm *leaves, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t w[8]; sc_load_words(w, leaves[i].v);
    leaves[i] = sc_from_words(w);
}
// every node of one level from the level below: one lane per parent, its two children are 64 contiguous bytes
__global__ void __launch_bounds__(256) k_merkle_level(scm *tree, uint32_t level, const scm *__restrict__ rc) {
    const uint32_t parents = 1u << level, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= parents) return;
    const uint32_t h = parents + t;
    const scm left = tree[2 * h], right = tree[2 * h + 1];
    tree[h] = mimc_node(left, right, rc);
}
// levels from_level .. 0 (2^from_level <= 256 parents) in one launch of ONE 256-lane block: a level reads what the level before wrote, so the levels are
// separated by a block barrier that every lane reaches - the loads and the store are guarded, the barrier is not.  This saves launches, not latency: each
// level is still a chain of 1,944 dependent products.
__global__ void __launch_bounds__(256) k_merkle_top(scm *tree, uint32_t from_level, const scm *__restrict__ rc) {
    for (int level = (int)from_level; level >= 0; level--) {
        const uint32_t parents = 1u << level;
        if (threadIdx.x < parents) {
            const uint32_t h = parents + threadIdx.x;
            const scm left = tree[2 * h], right = tree[2 * h + 1];
            tree[h] = mimc_node(left, right, rc);
        }
        __syncthreads();
    }
}
// the same node function over an explicit list of parent heap indices (the ancestors of updated leaves at one level; distinct, so no two lanes write one node)
__global__ void __launch_bounds__(256) k_merkle_level_list(scm *tree, const uint32_t *__restrict__ parents, uint32_t count, const scm *__restrict__ rc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t h = parents[t];
    const scm left = tree[2 * h], right = tree[2 * h + 1];
    tree[h] = mimc_node(left, right, rc);
}
// Trees that grow (bpg_merkle_build_partial, bpg_merkle_append): capacity 2^depth, `size` leaves, and every leaf from `size` on holds one `empty` value.  A
// subtree without a leaf is then one of depth + 1 constants - E[0] = empty, E[s + 1] = node(E[s], E[s]) - which the host computes (a chain of `depth`
// nodes is `depth` latency floors here and a millisecond there) and this kernel writes wherever they belong: one lane per heap node h >= 1; with L the
// level of h, j = h - 2^L its place in the level and s = depth - L its height, the subtree of h holds leaves [j 2^s, (j + 1) 2^s), so it is empty exactly
// when j >= ceil(size / 2^s).  Occupied nodes are left alone.  32 bytes per lane in two 16-byte stores; entry 0 of the array is no node.
__global__ void __launch_bounds__(256) k_merkle_fill_empty(scm *tree, uint32_t depth, uint32_t size, const scm *__restrict__ E) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;          // depth <= 24: the heap has at most 2^25 nodes, size <= 2^24
    if (h < 1u || h >= (2u << depth)) return;
    const uint32_t L = 31u - (uint32_t)__clz((int)h), j = h - (1u << L), s = depth - L;
    if (j < ((size + (1u << s) - 1u) >> s)) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(E[s].v);
    const uint4 a = src[0], b = src[1];
    uint4 *dst = reinterpret_cast<uint4 *>(tree[h].v);
    dst[0] = a; dst[1] = b;
}
// the node function of k_merkle_level over an interval of one level: lane t < count computes heap node first + t from its two children
__global__ void __launch_bounds__(256) k_merkle_level_range(scm *tree, uint32_t first, uint32_t count, const scm *__restrict__ rc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t h = first + t;
    const scm left = tree[2 * h], right = tree[2 * h + 1];
    tree[h] = mimc_node(left, right, rc);
}
// From the dirty children [lo, hi] of one level (2 <= lo <= hi, both of that level, at most BPG_MERKLE_TOP_PARENTS parents above them) to the root in one
// launch of ONE 256-lane block, as k_merkle_top goes: per level the interval halves, lane t <= hi - lo computes node lo + t, and a block barrier that every
// lane reaches separates the levels - the loads and the store are guarded, the barrier is not.  lo and hi are kernel arguments, so the trip count is
// uniform; an interval never widens on the way up.  The loop ends with the root (lo == hi == 1).
__global__ void __launch_bounds__(256) k_merkle_climb(scm *tree, uint32_t lo, uint32_t hi, const scm *__restrict__ rc) {
    do {
        lo >>= 1; hi >>= 1;
        if (threadIdx.x <= hi - lo) {
            const uint32_t h = lo + threadIdx.x;
            const scm left = tree[2 * h], right = tree[2 * h + 1];
            tree[h] = mimc_node(left, right, rc);
        }
        __syncthreads();
    } while (lo > 1u);
}
// new leaves of an update: leaf index[i] = raw[i] (32 bytes, any 256-bit value) in Montgomery form; the indices are distinct
__global__ void __launch_bounds__(256) k_merkle_set_leaves(scm *tree, uint32_t depth, const uint32_t *__restrict__ index, const uint32_t *__restrict__ raw, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t w[8]; sc_load_words(w, raw + 8 * (size_t)i);
    tree[(1u << depth) + index[i]] = sc_from_words(w);
}
// authentication paths: one thread per (item, level); out[item][lv] = the sibling of leaf index[item]'s ancestor lv levels above the leaves (lv = 0: the
// leaf's own sibling), canonical bytes.  ancestors != 0 (bpg_merkle_path_nodes): out[item][lv] = that ancestor's PARENT instead - the nodes ON the path, from
// the leaf's parent up to the root (lv = depth - 1), the values a path circuit computes where the siblings are what it is given
__global__ void __launch_bounds__(256) k_merkle_paths(const scm *__restrict__ tree, uint32_t depth, const uint32_t *__restrict__ index, uint32_t count, uint32_t ancestors,
                                                      uint32_t *__restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;          // count * depth < 2^32 (the engine cuts longer lists into several launches)
    if (t >= count * depth) return;
    const uint32_t item = t / depth, lv = t - item * depth;
    const uint32_t h = ((1u << depth) + index[item]) >> lv;            // lv < depth: h >= 2, so h >> 1 >= 1 is a node of the heap
    sc_store_canonical(out + 8 * (size_t)t, tree[ancestors ? h >> 1 : h ^ 1u]);
}
// a run of nodes as canonical bytes (bpg_merkle_root, bpg_merkle_nodes)
__global__ void __launch_bounds__(256) k_merkle_export(const scm *__restrict__ nodes, uint32_t count, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    sc_store_canonical(out + 8 * (size_t)i, nodes[i]);
}
#endif  // __HIPCC__

}  // namespace bpg
