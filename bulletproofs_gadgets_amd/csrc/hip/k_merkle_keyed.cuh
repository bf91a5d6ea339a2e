// MiMC Merkle trees in the keyed layout - part of kernels.cuh (included from there; see its header for the kernel map).  The layout, its invariant and every
// index rule are host/merkle_keyed_plan.hpp: height s = 0 is the leaves, s = depth the root, height s stores the cnt[s] nodes that have a held key below them
// as sorted positions pos[s] beside their values val[s], and a node that is not stored has the value E[s] of the (depth + 1)-scalar table the tree owns.
// Every lookup is a binary search of that header; nothing here computes an index of its own.  The node function and its constants are k_mimc.cuh's.
// A put runs in two phases separated by launches: the structure (k_mkx_classify, the three scan launches k_mkx_scan_sums / _scan_top / _scatter, k_mkx_merge),
// which hashes nothing, then the hashing (k_mkx_set_leaves, k_mkx_level per wide height, one k_mkx_climb).  No kernel hands anything to another workgroup
// of the same launch.
#pragma once
#include "k_mimc.cuh"
#include "k_merkle_prefix.cuh"     // mpx_copy32
#include "../host/merkle_keyed_plan.hpp"

namespace bpg {

// a keyed tree as the kernels that walk more than one height see it, by value; entries above `depth` are null
struct MkxView {
    const uint32_t *pos[MERKLE_KEYED_MAX_DEPTH + 1];
    scm *val[MERKLE_KEYED_MAX_DEPTH + 1];
    uint32_t cnt[MERKLE_KEYED_MAX_DEPTH + 1];
    uint32_t depth;
};
// the dirty lists of a put, by value: list[s] holds the m[s] dirty positions of height s, ascending
struct MkxDirty {
    const uint32_t *list[MERKLE_KEYED_MAX_DEPTH + 1];
    uint32_t m[MERKLE_KEYED_MAX_DEPTH + 1];
};

#if defined(__HIPCC__)
static_assert(MERKLE_KEYED_SCAN_TILE == 4 * 256, "the scan kernels cover four flags per lane of a 256-lane block");

// node (s, p) wherever it lives: its stored value, or the table's constant (such a node has no held key below it)
__device__ __forceinline__ scm mkx_read(const uint32_t *pos, const scm *val, uint32_t cnt, const scm *Es, uint64_t p) {
    const uint32_t r = merkle_keyed_find(pos, cnt, p);
    return r != MERKLE_KEYED_ABSENT ? val[r] : *Es;
}
// parent p of the height above (cpos, cval, ccnt): its two children by lookup, a missing child = *Es; the value goes to p's own slot, found by lookup
__device__ __forceinline__ void mkx_node(const uint32_t *cpos, const scm *cval, uint32_t ccnt, const uint32_t *ppos, scm *pval, uint32_t pcnt, uint32_t p, const scm *Es,
                                         const scm *__restrict__ rc) {
    uint32_t li, ri;
    merkle_keyed_children(cpos, ccnt, p, &li, &ri);
    const uint32_t at = merkle_keyed_find(ppos, pcnt, p);
    if (at == MERKLE_KEYED_ABSENT) return;              // (the structure phase stored every dirty position: this does not happen)
    const scm left = li != MERKLE_KEYED_ABSENT ? cval[li] : *Es, right = ri != MERKLE_KEYED_ABSENT ? cval[ri] : *Es;
    pval[at] = mimc_node(left, right, rc);
}
// inclusive scan of one uint2 per lane over the 256 lanes of a block (componentwise); every lane of the block calls it; lds holds 256 entries
__device__ __forceinline__ uint2 mkx_block_scan(uint2 v, uint2 *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        uint2 add = make_uint2(0, 0);
        if (threadIdx.x >= d) add = lds[threadIdx.x - d];
        __syncthreads();
        v.x += add.x; v.y += add.y;
        lds[threadIdx.x] = v;
        __syncthreads();
    }
    return v;
}

// classify + head flags, one lane per dirty position of one height: flags[i].x = 1 when dirty[i] is brand-new (not among the cnt stored positions; 0 when
// classify == 0: above the first height without a brand-new position nothing is), flags[i].y = 1 when entry i starts a new parent (0 when derive == 0: the root)
__global__ void __launch_bounds__(256) k_mkx_classify(const uint32_t *__restrict__ pos, uint32_t cnt, const uint32_t *__restrict__ dirty, uint32_t m, uint32_t classify,
                                                      uint32_t derive, uint2 *__restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint2 f;
    f.x = (classify && merkle_keyed_is_new(pos, cnt, dirty[i])) ? 1u : 0u;
    f.y = (derive && merkle_keyed_head(dirty, i)) ? 1u : 0u;
    flags[i] = f;
}
// scan, first launch: sums[b] = the sum of the flags of tile b (MERKLE_KEYED_SCAN_TILE flags, four consecutive ones per lane)
__global__ void __launch_bounds__(256) k_mkx_scan_sums(const uint2 *__restrict__ flags, uint32_t m, uint2 *__restrict__ sums) {
    __shared__ uint2 lds[256];
    const uint32_t base = blockIdx.x * MERKLE_KEYED_SCAN_TILE + 4u * threadIdx.x;
    uint2 v = make_uint2(0, 0);
    for (uint32_t k = 0; k < 4; k++)
        if (base + k < m) { const uint2 f = flags[base + k]; v.x += f.x; v.y += f.y; }
    v = mkx_block_scan(v, lds);
    if (threadIdx.x == 255) sums[blockIdx.x] = v;
}
// scan, second launch, ONE block: the tile sums become their exclusive scan in place, 256 at a time with a running carry; totals[0] = the two totals
__global__ void __launch_bounds__(256) k_mkx_scan_top(uint2 *sums, uint32_t tiles, uint2 *__restrict__ totals) {
    __shared__ uint2 lds[256];
    uint2 carry = make_uint2(0, 0);
    for (uint32_t base = 0; base < tiles; base += 256) {                // `tiles` is a kernel argument: every lane makes the same trips and reaches every barrier
        const uint32_t i = base + threadIdx.x;
        const uint2 own = i < tiles ? sums[i] : make_uint2(0, 0);
        const uint2 inc = mkx_block_scan(own, lds);
        if (i < tiles) sums[i] = make_uint2(carry.x + inc.x - own.x, carry.y + inc.y - own.y);
        const uint2 all = lds[255];
        carry.x += all.x; carry.y += all.y;
        __syncthreads();                                                // lds is written again by the next trip
    }
    if (threadIdx.x == 0) totals[0] = carry;
}
// scan, third launch: every flag's exclusive rank = the tile's offset + the rank inside the tile; a brand-new position goes to fresh[rank.x], the parent of a
// head to next[rank.y].  fresh and next have room for every flag set (the engine sizes them by m); either may be null when its flags are all zero.
__global__ void __launch_bounds__(256) k_mkx_scatter(const uint32_t *__restrict__ dirty, const uint2 *__restrict__ flags, uint32_t m, const uint2 *__restrict__ sums,
                                                     uint32_t *__restrict__ fresh, uint32_t *__restrict__ next) {
    __shared__ uint2 lds[256];
    const uint32_t base = blockIdx.x * MERKLE_KEYED_SCAN_TILE + 4u * threadIdx.x;
    uint2 f[4], v = make_uint2(0, 0);
    for (uint32_t k = 0; k < 4; k++) {
        f[k] = base + k < m ? flags[base + k] : make_uint2(0, 0);
        v.x += f[k].x; v.y += f[k].y;
    }
    const uint2 inc = mkx_block_scan(v, lds), off = sums[blockIdx.x];
    uint2 at = make_uint2(off.x + inc.x - v.x, off.y + inc.y - v.y);
    for (uint32_t k = 0; k < 4; k++) {
        if (base + k >= m) break;
        const uint32_t p = dirty[base + k];
        if (f[k].x && at.x < m) fresh[at.x] = p;
        if (f[k].y && at.y < m) next[at.y] = p >> 1;
        at.x += f[k].x; at.y += f[k].y;
    }
}
// merge: the cnt old entries and the n_new brand-new positions of one height into arrays of cnt + n_new entries (not the old ones), one lane per old entry
// and one per brand-new one; an old entry keeps its value, a brand-new one holds *Es until the hashing (or k_mkx_set_leaves) writes it
__global__ void __launch_bounds__(256) k_mkx_merge(const uint32_t *__restrict__ pos, const scm *__restrict__ val, uint32_t cnt, const uint32_t *__restrict__ fresh, uint32_t n_new,
                                                   uint32_t *__restrict__ dpos, scm *__restrict__ dval, const scm *__restrict__ Es) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt) {
        const uint32_t p = pos[t], at = merkle_keyed_old_dest(t, p, fresh, n_new);
        if (at >= cnt + n_new) return;
        dpos[at] = p; mpx_copy32(dval + at, val + t);
    } else if (t - cnt < n_new) {
        const uint32_t k = t - cnt, p = fresh[k], at = merkle_keyed_new_dest(k, p, pos, cnt);
        if (at >= cnt + n_new) return;
        dpos[at] = p; mpx_copy32(dval + at, Es);
    }
}
// set-leaves: the leaf of key[i] = raw[i] (32 bytes, any 256-bit value) in Montgomery form; the keys are distinct and held (the structure phase stored them)
__global__ void __launch_bounds__(256) k_mkx_set_leaves(const uint32_t *__restrict__ pos, scm *__restrict__ val, uint32_t cnt, const uint32_t *__restrict__ key,
                                                        const uint32_t *__restrict__ raw, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t at = merkle_keyed_find(pos, cnt, key[i]);
    if (at == MERKLE_KEYED_ABSENT) return;
    uint32_t w[8]; sc_load_words(w, raw + 8 * (size_t)i);
    val[at] = sc_from_words(w);
}
// level: the m > 256 dirty parents of one height from their children in the height below, one lane per parent
__global__ void __launch_bounds__(256) k_mkx_level(const uint32_t *__restrict__ cpos, const scm *__restrict__ cval, uint32_t ccnt, const uint32_t *__restrict__ ppos, scm *__restrict__ pval,
                                                   uint32_t pcnt, const uint32_t *__restrict__ dirty, uint32_t m, const scm *__restrict__ Es, const scm *__restrict__ rc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    mkx_node(cpos, cval, ccnt, ppos, pval, pcnt, dirty[t], Es, rc);
}
// climb: heights s + 1 .. depth, each with at most 256 dirty parents, in one launch of ONE 256-lane block.  A height reads what the height before wrote, so the
// heights are separated by a block barrier that every lane reaches - the lookups, the loads and the store are guarded, the barrier is not.  s and the depth are
// kernel arguments, so the trip count (up to 32) is uniform.
__global__ void __launch_bounds__(256) k_mkx_climb(MkxView V, MkxDirty D, uint32_t s, const scm *__restrict__ E, const scm *__restrict__ rc) {
    for (; s < V.depth; s++) {
        if (threadIdx.x < D.m[s + 1]) mkx_node(V.pos[s], V.val[s], V.cnt[s], V.pos[s + 1], V.val[s + 1], V.cnt[s + 1], D.list[s + 1][threadIdx.x], E + s, rc);
        __syncthreads();
    }
}
// paths: one thread per (item, lv), lv < depth; out[item][lv] = the sibling of key index[item]'s ancestor at height lv, canonical bytes; ancestors != 0: the
// ancestor at height lv + 1 instead (the nodes ON the path, the root last).  Any key below 2^depth, held or not.  Positions are 64 bits wide.
__global__ void __launch_bounds__(256) k_mkx_paths(MkxView V, const scm *__restrict__ E, const uint32_t *__restrict__ index, uint32_t count, uint32_t ancestors,
                                                   uint32_t *__restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;          // count * depth < 2^32 (the engine cuts longer lists into several launches)
    if (t >= count * V.depth) return;
    const uint32_t item = t / V.depth, lv = t - item * V.depth, s = ancestors ? lv + 1u : lv;
    const uint64_t a = merkle_keyed_ancestor(index[item], s), p = ancestors ? a : merkle_keyed_sibling(a);
    sc_store_canonical(out + 8 * (size_t)t, mkx_read(V.pos[s], V.val[s], V.cnt[s], E + s, p));
}
// export: nodes first .. first + count - 1 of one height as canonical bytes (bpg_merkle_root, bpg_merkle_nodes), each by lookup
__global__ void __launch_bounds__(256) k_mkx_export(const uint32_t *__restrict__ pos, const scm *__restrict__ val, uint32_t cnt, const scm *__restrict__ Es, uint64_t first,
                                                    uint32_t count, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    sc_store_canonical(out + 8 * (size_t)i, mkx_read(pos, val, cnt, Es, first + i));
}
// get: the leaf of key[i] as canonical bytes (E_0 for a key that is not held) and held[i] = 1 or 0
__global__ void __launch_bounds__(256) k_mkx_get(const uint32_t *__restrict__ pos, const scm *__restrict__ val, uint32_t cnt, const scm *__restrict__ E0, const uint32_t *__restrict__ key,
                                                 uint32_t count, uint32_t *__restrict__ out, uint8_t *__restrict__ held) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t r = merkle_keyed_find(pos, cnt, key[i]);
    sc_store_canonical(out + 8 * (size_t)i, r != MERKLE_KEYED_ABSENT ? val[r] : *E0);
    held[i] = r != MERKLE_KEYED_ABSENT ? 1 : 0;
}
// keys: held keys first .. first + count - 1 in ascending order, 64 bits each (first + count <= cnt)
__global__ void __launch_bounds__(256) k_mkx_keys(const uint32_t *__restrict__ pos, uint32_t first, uint32_t count, uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = pos[first + i];
}
// gather (bpg_merkle_get on a dense or prefix tree): leaf key[i] of a contiguous leaf array of `width` entries as canonical bytes; a key at or beyond the
// width (a prefix tree, right of its reserve) reads *E0
__global__ void __launch_bounds__(256) k_mkx_gather(const scm *__restrict__ leaves, uint64_t width, const scm *__restrict__ E0, const uint32_t *__restrict__ key, uint32_t count,
                                                    uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t k = key[i];
    sc_store_canonical(out + 8 * (size_t)i, k < width ? leaves[k] : *E0);
}
#endif  // __HIPCC__

}  // namespace bpg
