"""Keyed MiMC Merkle trees on the GPU (bpg_merkle_build_keyed, bpg_merkle_put, bpg_merkle_get, bpg_merkle_keys, bpg_merkle_node_counts and every other
bpg_merkle_* call on such a tree; the kernels of csrc/hip/k_merkle_keyed.cuh with the index rules of csrc/host/merkle_keyed_plan.hpp).

Up to depth 16 the reference is the dense tree of the padded list on the same device (Context.merkle_tree(padded, depth=...): code this layout does not
touch): every output is compared byte for byte - and again at depth 19, where a put has more than 256 scan tiles (section 10: the put scenarios of
tests/keyed_cases.py, compared whole).  At depth 32 it is the model of tests/keyed_cases.py, hashed by the oracle's sponge.  There are no tolerances.

The census of live resources is process-wide, so the scenario that ends with a census of zero runs in a child process: this file run as
`python tests/test_merkle_keyed_gpu.py child` prints one JSON line."""
import ctypes as C
import json
import pathlib
import subprocess
import sys

if __name__ == "__main__":
    _root = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "tests"), str(_root / "tests" / "golden")]

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import pyref as R
import gate_cases as G
import keyed_cases as K
from keyed_cases import le, red
from template_inputs_cases import rng

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
LC = bpg.LinearCombination
NODE_PRODUCTS = 2 * 2 * 486                                   # two blocks, 486 rounds, a square and a product per round
HASHING = ("k_mkx_level", "k_mkx_climb")
STRUCTURE = ("k_mkx_classify", "k_mkx_scan_sums", "k_mkx_scan_top", "k_mkx_scatter", "k_mkx_merge", "k_mkx_set_leaves")
OTHERS = ("k_merkle_fill_empty", "k_merkle_level_range", "k_merkle_climb", "k_merkle_level", "k_merkle_top", "k_merkle_level_list", "k_mpx_fill", "k_mpx_range", "k_mpx_climb", "k_mpx_list")
MIN_CAPACITY = 64                                             # MERKLE_KEYED_MIN_CAPACITY


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    yield c
    c.close()


def keyed(ctx, held, depth, empty=None, order=None):
    keys = list(held) if order is None else order
    return ctx.merkle_tree([held[k] for k in keys], depth=depth, empty=empty, keys=keys)


def dense(ctx, held, depth, empty=None):
    """the dense tree of the padded list: `empty` wherever no key is held"""
    return ctx.merkle_tree(K.padded(depth, held, empty), depth=depth, empty=empty)


def policy(cap, need, limit):
    """merkle_keyed_capacity of csrc/host/merkle_keyed_plan.hpp"""
    return cap if need <= cap else max(need, min(limit, max(MIN_CAPACITY, 2 * cap, need)))


def grown(caps, counts, depth):
    """the room per height after a put that leaves `counts` nodes stored"""
    return [policy(c, n, min(1 << (depth - s), 1 << 24)) for s, (c, n) in enumerate(zip(caps, counts))]


def held_bytes(caps, depth):
    return 36 * sum(caps) + 32 * (depth + 1)


def windows(depth, held):
    """per level (0 = the root) runs of up to four nodes around every stored position's edge: they straddle stored and absent nodes"""
    out = []
    for s in range(depth + 1):
        level, width = depth - s, 1 << (depth - s)
        stored = sorted({k >> s for k in held})
        for p in stored[:2] + stored[-2:] + [0, width - 1]:
            first = max(0, min(p - 1, width - 1))
            out.append((level, first, min(4, width - first)))
    return sorted(set(out))


def same_tree(t, d, held, indices, full=True):
    """every output of keyed tree t against dense tree d of the padded list"""
    depth = d.depth
    assert t.keyed and t.depth == depth and t.size == len(held) and t.capacity == d.capacity
    assert t.root() == d.root()
    if full:
        for level in range(depth + 1):
            assert t.nodes(level) == d.nodes(level), (sorted(held)[:8], level)
    for level, first, count in windows(depth, held):
        assert t.nodes(level, first, count) == d.nodes(level, first, count), (sorted(held)[:8], level, first)
    assert t.paths(indices) == d.paths(indices)
    assert t.path_nodes(indices) == d.path_nodes(indices)
    assert t.path_inputs(indices) == d.path_inputs(indices)
    all_leaves = d.nodes(depth)
    leaves, is_held = t.get(indices)
    assert leaves == [all_leaves[i] for i in indices] and is_held == [i in held for i in indices]
    assert t.keys() == sorted(held)
    counts, nbytes = t.node_counts
    assert counts == K.counts_of(held, depth)
    assert nbytes >= 36 * sum(counts) + 32 * (depth + 1) and t.reserved == (len(held), nbytes)


def logged(ctx, fn):
    """fn() under the all-kernels profile -> (its result, launches, node evaluations) per kernel"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    names = HASHING + STRUCTURE + OTHERS
    return res, {k: rep.get(k, {}).get("count", 0) for k in names}, {k: rep.get(k, {}).get("field_mults", 0) / NODE_PRODUCTS for k in names}


def check_log(count, evals, keys, depth, want=None):
    """what a put of `keys` launches and hashes: the model's evaluations (`want`, where the caller has them already); one launch per height above 256 dirty
    parents, and one climb"""
    want = want or (K.evals_of(keys, depth) if keys else [0] * depth)
    assert evals["k_mkx_level"] + evals["k_mkx_climb"] == sum(want), (evals, want)
    assert evals["k_mkx_level"] == sum(m for m in want if m > K.TOP)
    assert count["k_mkx_level"] + count["k_mkx_climb"] == K.hashing_launches(want), (count, want)
    assert count["k_mkx_climb"] == (1 if keys else 0) and count["k_mkx_set_leaves"] == (1 if keys else 0)
    for k in OTHERS:
        assert count[k] == 0, (k, count)


# ---------------------------------------------------------------------------------------------------------------- 1, 2: every subset of a small tree
@pytest.mark.parametrize("which", range(3))
def test_depth3_every_subset(ctx, which):
    depth, idx = 3, list(range(8))
    for mask in range(256):
        if mask % 3 != which:
            continue
        empty = K.EMPTIES[(mask // 3) % 3]
        keys = [k for k in range(7, -1, -1) if mask >> k & 1]                # descending: the host sorts
        held = {k: K.leaf_of(k) for k in keys}
        if not keys:                                                         # the empty set launches no node function
            t, count, evals = logged(ctx, lambda: keyed(ctx, held, depth, empty))
            assert sum(count.values()) == 0 and sum(evals.values()) == 0 and t.root() == K.empty_chain(depth, empty)[depth]
        else:
            t = keyed(ctx, held, depth, empty)
        d = dense(ctx, held, depth, empty)
        same_tree(t, d, held, idx)
        assert t.empty_nodes() == d.empty_nodes() == K.empty_chain(depth, empty)
        t.free(); d.free()


def test_depth1_every_subset(ctx):
    """the root's children are the leaves"""
    for mask in range(4):
        for empty in K.EMPTIES:
            held = {k: K.leaf_of(k + 5) for k in range(2) if mask >> k & 1}
            t = keyed(ctx, held, 1, empty)
            d = dense(ctx, held, 1, empty)
            same_tree(t, d, held, [0, 1])
            assert t.root() == K.node(red(held.get(0, empty or bytes(32))), red(held.get(1, empty or bytes(32))))
            t.free(); d.free()


# ---------------------------------------------------------------------------------------------------------------- 3: chosen sets
SETS = {depth: K.chosen_sets(depth) for depth in (10, 13)}


@pytest.mark.parametrize("depth,name", [(depth, name) for depth in (10, 13) for name in SETS[depth]])
def test_chosen_sets(ctx, depth, name):
    keys = SETS[depth][name]
    leaves = K.rand_scalars(b"chosen %d %s" % (depth, name.encode()), len(keys))
    held = dict(zip(keys, leaves))
    empty = K.EMPTIES[len(name) % 3]
    t, count, evals = logged(ctx, lambda: keyed(ctx, held, depth, empty, order=keys))
    check_log(count, evals, keys, depth)
    d = dense(ctx, held, depth, empty)
    n = 1 << depth
    idx = sorted({i for k in keys[:40] + sorted(keys)[:3] + sorted(keys)[-3:] for i in (k - 1, k, k + 1) if 0 <= i < n} | {0, n - 1, n // 2 - 1, n // 2})
    same_tree(t, d, held, idx)
    t.free(); d.free()


# ---------------------------------------------------------------------------------------------------------------- 4: put sequences
def run_sequence(ctx, depth, start, steps, empty=None):
    """a keyed tree of `start`, then every step (keys, kind) as one put: compared with a dense tree of the same padded list after every step, its launch log
    against the model; kind: "held" (no merge at any height), "new" or "mixed"."""
    held = {k: K.leaf_of(k) for k in start}
    t = keyed(ctx, held, depth, empty, order=list(start))
    n = 1 << depth
    for r, (keys, kind) in enumerate(steps):
        leaves = K.rand_scalars(b"step %d %d" % (depth, r), len(keys))
        fresh = [k for k in keys if k not in held]
        assert {"held": not fresh, "new": len(fresh) == len(keys), "mixed": 0 < len(fresh) < len(keys)}[kind], (r, kind)
        caps_before = t.node_counts[1]
        (inserted, root), count, evals = logged(ctx, lambda: t.put(keys, leaves, return_root=True))
        held.update(zip(keys, leaves))
        assert inserted == len(fresh)
        check_log(count, evals, keys, depth)
        # merges: one per height that gains a position, none above the first height that gains none
        gains = [len({k >> s for k in fresh} - {k >> s for k in set(held) - set(fresh)}) for s in range(depth + 1)]
        assert count["k_mkx_merge"] == sum(1 for g in gains if g), (count, gains)
        if kind == "held":
            assert count["k_mkx_merge"] == 0 and t.node_counts[1] == caps_before
        d = dense(ctx, held, depth, empty)
        assert root == d.root()
        idx = sorted({i for k in keys[:24] for i in (k - 1, k, k + 1) if 0 <= i < n} | {0, n - 1})
        same_tree(t, d, held, idx)
        d.free()
    return t, held


def test_put_sequences_depth10(ctx):
    depth, n = 10, 1 << 10
    start = SETS[10]["random 300"][:100]
    lo, hi = min(start), max(start)
    mid = [k for k in range(lo + 1, hi) if k not in start][:5]
    steps = [
        (start[:7], "held"),                                                 # no merge at any height
        ([k for k in range(lo) if k not in start][:3], "new"),               # before all held keys
        ([k for k in range(n - 1, hi, -1)][:3], "new"),                      # after all
        (mid, "new"),                                                        # between
        (start[10:14] + [k for k in range(hi - 40, hi) if k not in start and k not in mid][:4], "mixed"),
        (start[:1], "held"),
    ]
    t, held = run_sequence(ctx, depth, start, steps, le(R.L - 1))
    t.free()


def test_put_outgrows_capacity_depth10(ctx):
    """60 keys sit in arrays of the minimum capacity, 64 (less where a height cannot hold as many); five more make height 0 outgrow it: arrays of twice the
    room there, and the bytes held are the policy's at every height"""
    depth = 10
    start = sorted(SETS[10]["random 300"][100:160])
    t, held = run_sequence(ctx, depth, start, [], None)
    counts, nbytes = t.node_counts
    caps = grown([0] * (depth + 1), counts, depth)
    assert counts[0] == 60 and caps[0] == MIN_CAPACITY and caps[depth] == 1 and nbytes == held_bytes(caps, depth)
    more = [k for k in SETS[10]["random 300"][160:] if k not in held][:5]
    t.free()
    t, held = run_sequence(ctx, depth, start, [(more, "new")], None)
    counts, nbytes = t.node_counts
    caps = grown(caps, counts, depth)
    assert counts[0] == 65 and caps[0] == 2 * MIN_CAPACITY and nbytes == held_bytes(caps, depth)
    t.free()


def test_put_600_scattered_keys_depth12(ctx):
    """600 scattered keys into a tree of 300: heights with more than 256 dirty parents are launches of their own; then 256 and 257 dirty parents at height 1,
    the two sides of that rule"""
    depth, n = 12, 1 << 12
    base = K.rand_keys(b"d12 base", 300, depth)
    scattered = [k for k in K.rand_keys(b"d12 scattered", 700, depth) if k not in base][:600]
    assert sum(1 for m in K.evals_of(scattered, depth) if m > K.TOP) >= 2
    t, held = run_sequence(ctx, depth, base, [(scattered, "new")], le(3))
    at256 = [2 * j + 1 for j in range(256)]                                  # 256 parents at height 1: the climb alone
    at257 = [2 * j for j in range(1000, 1257)]                               # 257 (and 129 above them): one launch for height 1, then the climb
    for keys, launches in ((at256, 1), (at257, 2)):
        assert K.hashing_launches(K.evals_of(keys, depth)) == launches
        leaves = K.rand_scalars(b"sides %d" % len(keys), len(keys))
        _, count, evals = logged(ctx, lambda: t.put(keys, leaves))
        held.update(zip(keys, leaves))
        check_log(count, evals, keys, depth)
        assert count["k_mkx_level"] == launches - 1 and count["k_mkx_climb"] == 1
    d = dense(ctx, held, depth, le(3))
    same_tree(t, d, held, [0, 1, 2, 1023, 1024, 1028, n - 1])
    t.free(); d.free()


# ---------------------------------------------------------------------------------------------------------------- 10: put scenarios, the WHOLE tree after every step
# The scenarios of keyed_cases (tiles_mixed, in_place, second_trip); test_merkle_keyed_host.py asserts on the CPU that each reaches the device path it is
# for.  A brand-new position that the scan ranks one slot off lands in the middle of a tile, so nothing here is sampled at depth 13.
def whole_tree(t, d, held, caps, depth):
    """every node, every key and every leaf of keyed tree t against dense tree d of the padded list, and the bytes held against the capacity policy"""
    n = 1 << depth
    same_tree(t, d, held, sorted({i for k in sorted(held)[::97] for i in (k - 1, k, k + 1) if 0 <= i < n} | {0, n - 1}), full=True)
    leaves, is_held = t.get(range(n))
    assert leaves == d.nodes(depth) and is_held == [k in held for k in range(n)]
    assert t.node_counts[1] == held_bytes(caps, depth)


def run_scenario(ctx, sc, empty):
    """a keyed tree over the scenario's base, then every put of it, compared whole after every step; -> the merge kinds of every put, height by height"""
    depth = sc.depth
    held = {k: K.leaf_of(k) for k in sc.base}
    t = keyed(ctx, held, depth, empty, order=list(sc.base))
    caps = K.capacities([0] * (depth + 1), K.counts_of(held, depth), depth)
    d = dense(ctx, held, depth, empty)
    whole_tree(t, d, held, caps, depth)
    d.free()
    seen = []
    for r, (keys, kind) in enumerate(sc.puts):
        keys = list(keys)
        leaves = K.rand_scalars(b"scenario %s %d" % (sc.name.encode(), r), len(keys))
        assert K.kind_of(held, keys) == kind
        lists, before = K.put_lists(held, keys, depth), K.counts_of(held, depth)
        (inserted, root), count, evals = logged(ctx, lambda: t.put(keys, leaves, return_root=True))
        held.update(zip(keys, leaves))
        kinds, caps = K.merge_kinds(caps, before, K.counts_of(held, depth), depth)
        seen.append(kinds)
        assert inserted == lists[0][1]
        check_log(count, evals, keys, depth)
        assert count["k_mkx_merge"] == sum(1 for k in kinds if k) == sum(1 for _, fresh in lists if fresh), (count, kinds)
        assert count["k_mkx_classify"] == count["k_mkx_scan_sums"] == count["k_mkx_scan_top"] == count["k_mkx_scatter"] == depth      # one of each per height below the root
        d = dense(ctx, held, depth, empty)
        assert root == d.root()
        whole_tree(t, d, held, caps, depth)
        d.free()
    t.free()
    return seen


@pytest.mark.parametrize("last", ["new", "held"])
def test_tiles_mixed_depth13(ctx, last):
    """ONE put of 4,097 sorted keys into a tree of 3,416: brand-new flags by scan tile none / all / irregular / irregular / one flag, so the rank of a
    brand-new key is its tile's offset (0, 0, 1,024, 1,466, 1,927) plus an irregular rank inside the tile; height 1 finds nothing brand-new and from height
    2 on the flags are written without a lookup (classify == 0) over a list of 1,594 positions, two tiles"""
    kinds, = run_scenario(ctx, K.tiles_mixed(last), le(R.L - 7))
    assert kinds == ["grows"] + [None] * 13                                  # (3,416 + 1,928 or 1,927 leaves outgrow the room for 3,416)


def test_in_place_depth13(ctx):
    """3,000 keys, 1,500 new ones that retire the arrays of heights 0..3, then 1,000 mixed keys that merge in the context's scratch at heights 0, 1 and 2:
    totals of 5,000, 3,511 and 2,014 entries, so every height splits the scratch (values first, positions behind them) at another place, over 20, 14 and 8 blocks"""
    seen = run_scenario(ctx, K.in_place(), None)
    assert seen == [["grows"] * 4 + [None] * 10, ["in place"] * 3 + [None] * 11]


def oracle_root(depth, key, leaf, siblings):
    """the root that the oracle's sponge gives a leaf and its path: `depth` hashes"""
    cur = leaf
    for s in range(depth):
        cur = O.mimc_sponge(siblings[s] + cur) if key >> s & 1 else O.mimc_sponge(cur + siblings[s])
    return cur


@pytest.mark.parametrize("last", ["new", "held"])
def test_second_trip_depth19(ctx, last):
    """2^17 keys, then put A of 262,144 keys (256 tile sums: one trip of k_mkx_scan_top) and put B of 262,145 (257: the second trip scans one tile of one
    flag on top of the carry of the first 256), both with mixed flags.  The reference is the dense tree of this device over the 2^19 padded list, and for
    the probe keys the oracle's sponge along get() and paths().  Leaves are 252 random bits, kept as one array of 2^19 rows beside a mask of held keys."""
    import numpy as np
    sc = K.second_trip(last)
    depth, n, empty = sc.depth, 1 << sc.depth, le(R.L - 19)
    rs = np.random.RandomState(1900 + len(last))

    def fresh_leaves(count):
        a = np.frombuffer(rs.bytes(32 * count), dtype=np.uint8).reshape(count, 32).copy()
        a[:, 31] &= 0x0f
        return a
    table, mask = np.tile(np.frombuffer(empty, dtype=np.uint8), (n, 1)), np.zeros(n, dtype=bool)
    base = np.array(sc.base)
    table[base], mask[base] = fresh_leaves(len(base)), True
    t = ctx.merkle_tree(table[base].tobytes(), depth=depth, empty=empty, keys=sc.base)
    caps = K.capacities([0] * (depth + 1), K.counts_np(base, depth), depth)
    for r, (keys, kind) in enumerate(sc.puts):
        keys, order = list(keys), sorted(keys)
        ka = np.array(keys)
        lists, before = K.put_lists_np(np.flatnonzero(mask), ka, depth), K.counts_np(np.flatnonzero(mask), depth)
        prev = mask.copy()
        leaves = fresh_leaves(len(keys))
        (inserted, root), count, evals = logged(ctx, lambda: t.put(keys, leaves.tobytes(), return_root=True))
        table[ka], mask[ka] = leaves, True
        now = np.flatnonzero(mask)
        after = K.counts_np(now, depth)
        kinds, caps = K.merge_kinds(caps, before, after, depth)
        assert inserted == lists[0][1] and 0 < inserted < len(keys) and kind == "mixed"
        check_log(count, evals, keys, depth, want=[m for m, _ in lists[1:]])
        assert count["k_mkx_merge"] == sum(1 for k in kinds if k) and count["k_mkx_scan_top"] == depth
        d = ctx.merkle_tree(table.tobytes(), depth=depth, empty=empty)
        assert root == d.root() == t.root()
        assert t.size == len(now) and t.keys() == now.tolist()
        counts, nbytes = t.node_counts
        assert counts == after and nbytes == held_bytes(caps, depth)
        for level in range(13):                                              # whole levels from the root down to level 12
            assert t.nodes(level) == d.nodes(level), (r, level)
        # the lowest levels: 4,096 nodes around the ancestors of the keys at the end of the dirty list (indices 262,143 and 262,144 of put B), of the key in
        # the middle of it, and of the first one
        for level in range(13, depth + 1):
            width = 1 << level
            for k in (order[-1], order[len(order) // 2], order[0]):
                first = max(0, min((k >> (depth - level)) - 2048, width - 4096))
                assert t.nodes(level, first, 4096) == d.nodes(level, first, 4096), (r, level, first)
        got, is_held = t.get(keys)                                           # every put key holds its leaf
        assert b"".join(got) == leaves.tobytes() and all(is_held)
        # the oracle, directly: held, brand-new and absent keys; the last keys of the sorted put and their neighbours
        absent = [int(k) for k in np.flatnonzero(~mask)[[0, -1]]]
        probe = sorted(set(order[-2:] + [k ^ 1 for k in order[-2:]] + [order[0], order[len(order) // 2], next(k for k in order if prev[k]), next(k for k in order if not prev[k])]
                           + absent + [int(base[0])]))
        got, is_held = t.get(probe)
        assert is_held == [bool(mask[k]) for k in probe] and got == [table[k].tobytes() if mask[k] else red(empty) for k in probe]
        if r == 1:
            assert bool(prev[order[-1]]) == (last == "held") and not prev[order[-2]]
        for k, leaf, sib in zip(probe, got, t.paths(probe)):
            assert oracle_root(depth, k, leaf, sib) == root, (r, k)
        d.free()
    t.free()


# ---------------------------------------------------------------------------------------------------------------- 5: depth 32 against the model
def check_deep(t, m, probe):
    depth = m.depth
    assert t.size == len(m.keys()) and t.keys() == m.keys() and t.root() == m.root() and t.empty_nodes() == m.E
    assert t.node_counts[0] == m.counts()
    assert t.paths(probe) == [m.siblings(i) for i in probe]
    assert t.path_nodes(probe) == [m.on_path(i) for i in probe]
    assert t.path_inputs(probe) == [bpg.merkle_path_inputs(i, m.siblings(i), m.root()) for i in probe]
    assert t.get(probe) == m.get(probe)
    assert t.nodes(0) == [m.root()] and t.nodes(1) == m.level(1) and t.nodes(2) == m.level(2)
    for k in m.keys()[:3] + m.keys()[-3:]:
        first = max(0, k - 1)
        assert t.nodes(depth, first, min(3, (1 << depth) - first)) == m.level(depth, first, min(3, (1 << depth) - first))


def test_depth32_against_the_model(ctx):
    depth, empty = 32, le(R.L - 2)
    keys = K.DEEP_KEYS + K.rand_keys(b"deep", 10, depth)                     # 16 keys
    assert len(set(keys)) == 16
    leaves = K.rand_scalars(b"deep leaves", 16)
    far = [12345, 2**31 + 7, 2**32 - 77777]
    probe = sorted({i for k in keys for i in (k - 1, k, k + 1) if 0 <= i < 1 << depth} | set(far))
    m = K.KeyedModel(depth, empty)
    m.put(keys, leaves)
    t = ctx.merkle_tree(leaves, depth=depth, empty=empty, keys=keys)        # in one call
    check_deep(t, m, probe)
    one = ctx.merkle_tree([], depth=depth, empty=empty, keys=[])            # and again key by key
    assert one.root() == m.E[depth] and one.size == 0 and one.keys() == []
    for k, leaf in zip(keys, leaves):
        assert one.put([k], [leaf]) == 1
    check_deep(one, m, probe)
    assert one.node_counts[0] == t.node_counts[0]
    repl = keys[:6] + keys[-2:]                                              # replacements, in both trees: put, and update
    new_leaves = K.rand_scalars(b"deep again", len(repl))
    m.put(repl, new_leaves)
    assert t.put(repl, new_leaves) == 0
    one.update(repl, new_leaves)
    check_deep(t, m, probe); check_deep(one, m, probe)
    # a leaf equal to `empty` keeps the key held, and the nodes are those of the absent key
    m.put([keys[7]], [empty])
    assert t.put([keys[7]], [empty]) == 0 and t.get([keys[7]]) == ([red(empty)], [True]) and t.size == 16
    check_deep(t, m, probe)
    with pytest.raises(bpg.BpgError) as e:                                   # a key of 2^depth has no leaf
        t.put([1 << 32], [le(1)])
    assert e.value.status == 4
    with pytest.raises(bpg.BpgError) as e:
        t.paths([1 << 32])
    assert e.value.status == 4
    t.free(); one.free()


# ---------------------------------------------------------------------------------------------------------------- 6: one proof each way at depth 32
def membership(ctx, index, value, blinding, siblings, root, gated):
    """the statement "leaf `index` of the tree with this root holds x_leaf": the path circuit over a committed leaf and ONE more row, leaf - x_leaf = 0,
    against a public x_leaf.  gated: MerklePath256 with 4 * depth + 1 path inputs and x_leaf as one more public input (one circuit for every index);
    otherwise the reference gadget MerkleTree256 of this index's pattern with every public value baked in (what the oracle's verifier is given)."""
    t = bpg.Transcript(G.PATH_LABEL); p = bpg.Prover(ctx, t)
    com, var = p.commit(value, blinding)
    d = len(siblings)
    if gated:
        xs = [p.input(v) for v in bpg.merkle_path_inputs(index, siblings, root) + [value]]
        bpg.MerklePath256(xs[4 * d], var, [tuple(xs[4 * j:4 * j + 4]) for j in range(d)]).prove(p, [], [])
        p.constrain(LC.of(var) - LC.of(xs[4 * d + 1]))
    else:
        pat, order = G.reference_pattern(index, d)
        bpg.MerkleTree256(root, [siblings[k] for k in order], [LC.of(var)], pat).prove(p, [], [])
        p.constrain(LC.of(var) - LC.of(value))
    return p, t, com


@pytest.fixture(scope="module")
def proofs32():
    """a context of its own with 2^16 generators, a depth-32 keyed tree, ONE template, and one wave of two proofs: a held key with its leaf, an absent key
    with `empty` - inputs and checkpoints from the tree's path_inputs and path_nodes"""
    from test_gates_gpu import state_before, _after_commit, to_oracle
    cap, depth, empty = 1 << 16, 32, le(R.L - 3)
    ctx = bpg.Context(0)
    ctx.gens_ensure(cap)
    keys = [2**31 - 1, 2**32 - 1, 0, 123456789]
    leaves = K.rand_scalars(b"proofs32", len(keys))
    tree = ctx.merkle_tree(leaves, depth=depth, empty=empty, keys=keys)
    idx = [2**31 - 1, 2**31]                                                 # held; absent, and the held key's neighbour across the middle of the tree
    values = [leaves[0], red(empty)]
    assert tree.get(idx) == (values, [True, False])
    root, paths, nodes = tree.root(), tree.paths(idx), tree.path_nodes(idx)
    inputs = [ins + [values[k]] for k, ins in enumerate(tree.path_inputs(idx))]
    p0, _, _ = membership(ctx, idx[0], values[0], G.blind("keyed", 0), paths[0], root, True)
    tmpl = p0.template(ctx, checkpoints=G.node_checkpoints(p0))
    pre = state_before(G.PATH_LABEL)
    res = tmpl.prove_batch_inputs([(values[k], [], pre, G.blind("keyed", k), rng("keyed %d" % k), 0, nodes[k], inputs[k]) for k in range(2)], commit=True)
    after = [_after_commit(pre, r[2]) for r in res]
    yield dict(ctx=ctx, tmpl=tmpl, res=res, after=after, inputs=inputs, idx=idx, values=values, paths=paths, root=root, cap=cap, to_oracle=to_oracle)
    tmpl.free(); tree.free(); ctx.close()


def test_depth32_membership_and_non_membership(proofs32):
    s = proofs32
    res, after, inputs = s["res"], s["after"], s["inputs"]
    assert all(r[0] is not None for r in res)
    item = lambda k, ins: (after[k], res[k][2], res[k][0], None, 0, None, b"".join(ins))
    st, _ = s["tmpl"].verify_batch([item(0, inputs[0]), item(1, inputs[1])])
    assert st == [0, 0], st                                                  # the GPU verifier accepts the held key's proof and the absent key's
    st, _ = s["tmpl"].verify_batch([item(1, inputs[0]), item(0, inputs[1])])
    assert st[0] != 0 and st[1] != 0, st                                     # the absent key's proof under the held key's inputs is rejected (and the other way)
    gens = O.Gens(s["cap"])
    for k in range(2):                                                       # the oracle's verifier, on the reference assembly of that index with the values baked in
        p, t, com = membership(s["ctx"], s["idx"][k], s["values"][k], G.blind("keyed", k), s["paths"][k], s["root"], False)
        assert com == res[k][2] and t.state == after[k]
        assert O.verify(gens, t.state, s["to_oracle"](p.instance()), com, res[k][0]) == 0, "the oracle's verifier rejects proof %d" % k
    p, t, com = membership(s["ctx"], s["idx"][0], s["values"][0], G.blind("keyed", 1), s["paths"][0], s["root"], False)
    assert O.verify(gens, after[1], s["to_oracle"](p.instance()), res[1][2], res[1][0]) != 0     # and the absent key's proof against the held key's statement


# ---------------------------------------------------------------------------------------------------------------- 7: refusals with a device
def test_refusals_with_a_device(ctx):
    depth = 10
    held = {k: K.leaf_of(k) for k in (5, 9, 700)}
    t = keyed(ctx, held, depth)
    state = lambda: (t.root(), t.node_counts, t.keys(), t.size)
    before = state()
    for keys in ([6], [5, 6], [1023]):                                       # update of a key that is not held: nothing changes
        with pytest.raises(bpg.BpgError) as e:
            t.update(keys, [le(1)] * len(keys))
        assert e.value.status == 4 and state() == before
    for call in (lambda: t.append([le(1)]), lambda: t.append([]), lambda: t.reserve(8), lambda: t.reserve(0), lambda: t.put([5, 5], [le(1), le(2)]), lambda: t.put([1024], [le(1)]),
                 lambda: t.get([1024]), lambda: t.keys(2, 2), lambda: t.keys(4, 0)):
        with pytest.raises(bpg.BpgError) as e:
            call()
        assert e.value.status == 4 and state() == before
    assert t.put([], []) == 0 and t.put([], [], return_root=True) == (0, before[0]) and t.keys(3, 0) == [] and state() == before
    t.update([9], [le(77)])                                                  # a held key: served
    assert t.get([9]) == ([le(77)], [True]) and t.root() != before[0]
    d = ctx.merkle_tree([le(1)] * 8, depth=4)
    p = ctx.merkle_tree([le(1)] * 3, depth=20, reserve=4)
    for other in (d, p):                                                     # put and node_counts refuse the other layouts
        root = other.root()
        for call in (lambda: other.put([1], [le(2)]), lambda: other.put([], []), lambda: other.node_counts):
            with pytest.raises(bpg.BpgError) as e:
                call()
            assert e.value.status == 4
        assert other.root() == root and not other.keyed
    lib = bpg.lib()
    ctx2 = bpg.Context(0)                                                    # a tree of another context
    ins, buf, held_b, ks, cnts, nb = C.c_uint64(0x5a5a), C.create_string_buffer(b"\x5a" * 32, 32), C.create_string_buffer(b"\x5a", 1), (C.c_uint64 * 1)(0x5a5a), (C.c_uint64 * 11)(*([0x5a5a] * 11)), C.c_uint64(0x5a5a)
    one = (C.c_uint64 * 1)(5)

    def every_call(c, tree):
        return [lib.bpg_merkle_put(c, tree._h, C.c_uint64(1), one, le(3), C.byref(ins), buf), lib.bpg_merkle_get(c, tree._h, C.c_uint64(1), one, buf, held_b),
                lib.bpg_merkle_keys(c, tree._h, C.c_uint64(0), C.c_uint64(1), ks), lib.bpg_merkle_node_counts(c, tree._h, cnts, C.byref(nb)),
                lib.bpg_merkle_update(c, tree._h, C.c_uint64(1), one, le(3)), lib.bpg_merkle_root(c, tree._h, buf)]
    untouched = lambda: ins.value == 0x5a5a and buf.raw == b"\x5a" * 32 and held_b.raw == b"\x5a" and ks[0] == 0x5a5a and list(cnts) == [0x5a5a] * 11 and nb.value == 0x5a5a
    now = state()
    assert every_call(ctx2._h, t) == [4] * 6 and untouched() and state() == now
    # a keyed tree after its context is closed: free alone is valid
    t2 = ctx2.merkle_tree([le(1), le(2)], depth=32, keys=[7, 2**32 - 1])
    assert t2.root() != t2.empty_nodes()[32]
    ctx2.close()
    assert every_call(ctx._h, t2) == [4] * 6 and untouched()
    t2.free()
    assert state() == now
    t.free(); d.free(); p.free()


# ---------------------------------------------------------------------------------------------------------------- 9: get and keys on the other layouts
def test_get_and_keys_on_dense_and_prefix_trees(ctx):
    leaves = K.rand_scalars(b"other layouts", 16)
    empty = le(11)
    trees = [(ctx.merkle_tree(leaves), 16), (ctx.merkle_tree(leaves[:5], depth=4, empty=empty), 5), (ctx.merkle_tree(leaves[:5], depth=4, empty=empty, reserve=6), 5),
             (ctx.merkle_tree(leaves[:3], depth=32, empty=empty, reserve=3), 3), (ctx.merkle_tree([], depth=4, empty=empty), 0)]
    for t, size in trees:
        depth = t.depth
        assert not t.keyed and t.size == size
        probe = [i for i in (0, 1, size - 1, size, size + 1, 7, (1 << depth) - 1) if 0 <= i < 1 << depth]
        got, held = t.get(probe)
        assert got == [t.nodes(depth, i, 1)[0] for i in probe] and held == [i < size for i in probe]
        assert t.keys() == list(range(size)) and t.keys(size, 0) == []
        if size > 1:
            assert t.keys(1, size - 1) == list(range(1, size)) and t.keys(size - 1) == [size - 1]
        with pytest.raises(bpg.BpgError) as e:
            t.keys(size, 1)
        assert e.value.status == 4
        with pytest.raises(bpg.BpgError) as e:
            t.get([1 << depth])
        assert e.value.status == 4
        t.free()


# ---------------------------------------------------------------------------------------------------------------- 8: the census (child process)
def case_census():
    """build, put until arrays are reallocated, free; a tree that outlives its context; the census at zero"""
    ok = {}
    ctx = bpg.Context(0)
    depth = 16
    keys = K.rand_keys(b"census", 700, depth)
    held = {k: K.leaf_of(k) for k in keys[:50]}
    t = ctx.merkle_tree([held[k] for k in keys[:50]], depth=depth, keys=keys[:50])
    sizes = [t.node_counts[1]]
    live = [bpg.live_resources()["device_buffers"]]
    for lo, hi in ((50, 70), (70, 200), (200, 700)):                        # 50 -> 70 -> 200 -> 700 keys: capacity 64, 128, 256 (or what is needed), 1024
        part = keys[lo:hi]
        held.update((k, K.leaf_of(k)) for k in part)
        ok["put %d" % hi] = t.put(part, [held[k] for k in part]) == hi - lo
        sizes.append(t.node_counts[1]); live.append(bpg.live_resources()["device_buffers"])
    ok["arrays were reallocated"] = sizes == sorted(sizes) and len(set(sizes)) == 4
    ok["no buffer is left behind by a reallocation"] = max(live) <= live[0] + 1                                    # (the scratch of a merge in place appears with the first one)
    d = ctx.merkle_tree(K.padded(depth, held), depth=depth)
    probe = sorted(held)[:5] + [0, 65535]
    ok["against the dense tree"] = t.root() == d.root() and t.paths(probe) == d.paths(probe) and t.keys() == sorted(held) and t.node_counts[0] == K.counts_of(held, depth)
    d.free()
    with_tree = bpg.live_resources()["device_buffers"]
    t.free()
    ok["free releases every array"] = bpg.live_resources()["device_buffers"] == with_tree - 2 * (depth + 1) - 1
    t = ctx.merkle_tree([le(1)], depth=32, keys=[2**32 - 1])                # a tree that outlives its context
    ctx.close()
    t.free()
    return {"ok": ok, "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}


def test_census_in_a_process_of_its_own():
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_merkle_keyed_gpu.py"), "child"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(out["ok"].values()), out
    assert out["end"] == [0] * 6, out


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    print(json.dumps(case_census()))
