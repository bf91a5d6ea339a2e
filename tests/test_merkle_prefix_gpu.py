"""MiMC Merkle trees in the prefix layout on the GPU (bpg_merkle_build_prefix, bpg_merkle_reserve, bpg_merkle_reserved and every other bpg_merkle_* call on
such a tree; the kernels of csrc/hip/k_merkle_prefix.cuh, launched from csrc/host/merkle_prefix_plan.hpp).

Up to depth 24 the reference is the dense tree of the same leaves on the same device (Context.merkle_tree without `reserve`: code this layout does not
touch, pinned by test_merkle_gpu.py and test_merkle_grow_gpu.py): every output is compared byte for byte.  Beyond depth 24 there is no dense tree, and the
reference is the oracle's sponge over the few nodes that are not constants (sparse_model below: a node without a leaf below it is E_s, computed by the
same sponge), with node() of test_merkle_grow_gpu.py remembering the pairs it has hashed.

bytes held = 32 x (sum over s = 0..depth of max(1, ceil(reserve / 2^s)) + depth + 1): the stored slots and the table of constants (held_bytes below).

The census of live resources is process-wide, so the scenario that ends with a census of zero runs in a child process: this file run as
`python tests/test_merkle_prefix_gpu.py child` prints one JSON line."""
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
import pyref as R
import gate_cases as G
from template_inputs_cases import rng
from test_merkle_grow_gpu import node, model, empty_chain, rand_scalars, le, red, all_levels, NODE_PRODUCTS
from test_gates_gpu import state_before, _after_commit

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
EMPTIES = [None, le(R.L - 1), le(2**256 - 1)]                  # NULL = zero, l - 1, and a value >= l: `empty` is taken mod l
PREFIX_KERNELS = ("k_mpx_fill", "k_mpx_range", "k_mpx_climb", "k_mpx_list", "k_mpx_set_leaves", "k_mpx_relayout")
DENSE_KERNELS = ("k_merkle_fill_empty", "k_merkle_level_range", "k_merkle_climb", "k_merkle_level", "k_merkle_top", "k_merkle_level_list", "k_merkle_set_leaves")
TOP = 256


def widths(depth, reserve):
    return [max(1, -(-reserve // (1 << s))) for s in range(depth + 1)]


def held_bytes(depth, reserve):
    return 32 * (sum(widths(depth, reserve)) + depth + 1)


def windows(depth, reserve):
    """per level (0 = the root) a window of up to three nodes that straddles the stored width W_s of its height"""
    out = []
    for s, w in enumerate(widths(depth, reserve)):
        level, first = depth - s, max(0, w - 1)
        out.append((level, first, min(3, (1 << level) - first)))
    return out


def same_tree(p, d, indices, reserve):
    """every output of prefix tree p against dense tree d of the same leaves"""
    depth = d.depth
    assert p.depth == depth and p.size == d.size and p.capacity == d.capacity
    assert p.root() == d.root()
    assert p.empty_nodes() == d.empty_nodes()
    for level in range(depth + 1):
        assert p.nodes(level) == d.nodes(level), (reserve, d.size, level)
    for level, first, count in windows(depth, reserve):
        assert p.nodes(level, first, count) == d.nodes(level, first, count), (reserve, d.size, level, first)
    assert p.paths(indices) == d.paths(indices), (reserve, d.size)
    assert p.path_nodes(indices) == d.path_nodes(indices), (reserve, d.size)
    assert p.path_inputs(indices) == d.path_inputs(indices), (reserve, d.size)
    assert p.reserved == (reserve, held_bytes(depth, reserve))


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def leaves12():
    """the leaves every test here takes a prefix of; nobody changes them"""
    return rand_scalars(b"prefix", 1500)


# ---------------------------------------------------------------------------------------------------------------- against the dense tree
@pytest.mark.parametrize("which", range(3))
def test_depth3_every_reserve_and_size(ctx, leaves12, which):
    empty, depth = EMPTIES[which], 3
    dense = {size: ctx.merkle_tree(leaves12[:size], depth=depth, empty=empty) for size in range(9)}
    for reserve in range(1, 9):
        for size in range(reserve + 1):
            p = ctx.merkle_tree(leaves12[:size], depth=depth, empty=empty, reserve=reserve)
            same_tree(p, dense[size], list(range(8)), reserve)
            p.free()
    for t in dense.values():
        t.free()


@pytest.mark.parametrize("reserve", [1, 3, 5, 1023, 1024])
def test_depth10(ctx, leaves12, reserve):
    depth = 10
    for k, size in enumerate(sorted({0, 1, reserve // 2, reserve - 1, reserve})):
        empty = EMPTIES[(k + reserve) % 3]
        d = ctx.merkle_tree(leaves12[:size], depth=depth, empty=empty)
        p = ctx.merkle_tree(leaves12[:size], depth=depth, empty=empty, reserve=reserve)
        # first and last leaf, both sides of the size, of the reserve and of every stored width on its way up
        idx = sorted({i for i in [0, 1, size - 1, size, reserve - 1, reserve, reserve + 1, 1023] + [(w << s) - 1 for s, w in enumerate(widths(depth, reserve))] +
                      [w << s for s, w in enumerate(widths(depth, reserve))] if 0 <= i < 1 << depth})
        same_tree(p, d, idx, reserve)
        p.free(); d.free()


# ---------------------------------------------------------------------------------------------------------------- the launch log
def logged(ctx, fn):
    """fn() under the all-kernels profile -> (its result, launches, node evaluations) of the tree kernels of both layouts"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    names = PREFIX_KERNELS + DENSE_KERNELS
    return res, {k: rep.get(k, {}).get("count", 0) for k in names}, {k: rep.get(k, {}).get("field_mults", 0) / NODE_PRODUCTS for k in names}


def check_log(count, evals, depth, old, new, build):
    """what growing a prefix tree from `old` to `new` leaves launches: the plan's launches and nothing else"""
    ancestors = [{i >> h for i in range(old, new)} for h in range(1, depth + 1)]
    wide = sum(1 for a in ancestors if len(a) > TOP)
    want = {"k_mpx_fill": 1 if build else 0, "k_mpx_range": wide, "k_mpx_climb": 1 if new > old else 0}
    for k in PREFIX_KERNELS + DENSE_KERNELS:
        assert count[k] == want.get(k, 0), (k, count)
    assert evals["k_mpx_range"] + evals["k_mpx_climb"] == sum(len(a) for a in ancestors), evals
    assert evals["k_mpx_range"] == sum(len(a) for a in ancestors if len(a) > TOP)
    assert evals["k_mpx_fill"] == 0


def test_wide_steps(ctx, leaves12):
    """depth 12, reserve 1,500 (odd widths at heights 2 and 3): 1,500 leaves are 750 and 375 parents in launches of their own, then the climb; 300 leaves at
    1,000 are 150 parents: the climb alone"""
    depth, reserve = 12, 1500
    p, count, evals = logged(ctx, lambda: ctx.merkle_tree(leaves12, depth=depth, reserve=reserve))
    check_log(count, evals, depth, 0, 1500, True)
    assert count["k_mpx_range"] == 2 and evals["k_mpx_range"] == 750 + 375
    d = ctx.merkle_tree(leaves12, depth=depth)
    assert all_levels(p) == all_levels(d)
    p.free(); d.free()
    p, count, evals = logged(ctx, lambda: ctx.merkle_tree(leaves12[:1000], depth=depth, reserve=reserve))
    check_log(count, evals, depth, 0, 1000, True)
    (first, root), count, evals = logged(ctx, lambda: p.append(leaves12[1000:1300], return_root=True))
    check_log(count, evals, depth, 1000, 1300, False)
    d = ctx.merkle_tree(leaves12[:1300], depth=depth)
    assert first == 1000 and root == d.root() and p.size == 1300 and p.reserved == (1500, held_bytes(depth, 1500))
    assert all_levels(p) == all_levels(d)
    _, count, evals = logged(ctx, lambda: (p.update([5, 1299], [le(1), le(2)]), d.update([5, 1299], [le(1), le(2)])))
    assert count["k_mpx_list"] == depth and count["k_mpx_set_leaves"] == 1 and evals["k_mpx_list"] == evals["k_merkle_level_list"] == 2 * depth - 2     # the paths meet below the root
    assert count["k_mpx_range"] == count["k_mpx_climb"] == count["k_mpx_fill"] == count["k_mpx_relayout"] == 0
    assert all_levels(p) == all_levels(d)
    p.free(); d.free()


# ---------------------------------------------------------------------------------------------------------------- regrow
def test_regrow(ctx, leaves12):
    """depth 5 from reserve 3: an append that outgrows the reserve takes min(32, max(2 R, size + count)) first - 6, 12, 32 - in one relayout launch"""
    depth, empty = 5, le(7)
    p = ctx.merkle_tree(leaves12[:3], depth=depth, empty=empty, reserve=3)
    assert p.reserved == (3, held_bytes(depth, 3)) == (3, 32 * (3 + 2 + 1 + 1 + 1 + 1 + 6))
    have = 3
    for add, reserve in ((1, 6), (4, 12), (24, 32)):
        (first, root), count, evals = logged(ctx, lambda: p.append(leaves12[have:have + add], return_root=True))
        assert count["k_mpx_relayout"] == 1 and count["k_mpx_climb"] == 1 and count["k_mpx_fill"] == 0
        have += add
        d = ctx.merkle_tree(leaves12[:have], depth=depth, empty=empty)
        assert first == have - add and root == d.root() and p.size == have
        same_tree(p, d, list(range(32)), reserve)
        d.free()
    assert have == 32 == p.capacity
    before = all_levels(p)
    with pytest.raises(bpg.BpgError) as e:                     # full: refused, and tree, size and reserve are as they were
        p.append([le(1)])
    assert e.value.status == 4 and p.size == 32 and p.reserved == (32, held_bytes(depth, 32)) and all_levels(p) == before
    p.free()
    # an explicit reserve: below the present one a no-op, above it one relayout that changes no node; beyond 2^depth refused
    p = ctx.merkle_tree(leaves12[:5], depth=depth, empty=empty, reserve=6)
    d = ctx.merkle_tree(leaves12[:5], depth=depth, empty=empty)
    _, count, _ = logged(ctx, lambda: (p.reserve(0), p.reserve(4), p.reserve(6)))
    assert sum(count.values()) == 0 and p.reserved == (6, held_bytes(depth, 6))
    _, count, _ = logged(ctx, lambda: p.reserve(9))
    assert count["k_mpx_relayout"] == 1 and sum(count.values()) == 1
    same_tree(p, d, list(range(32)), 9)
    for bad in (33, 1 << 24, (1 << 24) + 1):
        with pytest.raises(bpg.BpgError) as e:
            p.reserve(bad)
        assert e.value.status == 4
    with pytest.raises(bpg.BpgError) as e:                     # 5 + 28 > 32: refused before any regrow
        p.append(leaves12[:28])
    assert e.value.status == 4
    same_tree(p, d, list(range(32)), 9)
    p.free(); d.free()


def test_reserve_and_reserved_on_a_dense_tree(ctx, leaves12):
    for t, depth in ((ctx.merkle_tree(leaves12[:5], depth=4), 4), (ctx.merkle_tree(leaves12[:8]), 3)):
        assert t.reserved == (1 << depth, 32 * (2 << depth))
        before = all_levels(t)
        for n in (0, 1, 1 << depth, (1 << depth) + 1):
            with pytest.raises(bpg.BpgError) as e:
                t.reserve(n)
            assert e.value.status == 4
        assert all_levels(t) == before and t.reserved == (1 << depth, 32 * (2 << depth))
        t.free()
    with pytest.raises(bpg.BpgError) as e:                     # without the keyword depth 25 is refused as before
        ctx.merkle_tree(leaves12[:5], depth=25)
    assert e.value.status == 4
    with pytest.raises(ValueError):
        ctx.merkle_tree(leaves12[:4], reserve=4)


# ---------------------------------------------------------------------------------------------------------------- beyond the dense limit
class SparseModel:
    """the tree of depth `depth` over leaves || empty x (2^depth - len(leaves)) without its constants: value(s, j) of node j at height s (0 = the leaves)"""
    def __init__(self, leaves, depth, empty=None):
        self.leaves, self.depth, self.E = [red(x) for x in leaves], depth, empty_chain(depth, empty)

    def value(self, s, j):
        if j >= -(-len(self.leaves) // (1 << s)):
            return self.E[s]
        return self.leaves[j] if s == 0 else node(self.value(s - 1, 2 * j), self.value(s - 1, 2 * j + 1))

    def root(self):
        return self.value(self.depth, 0)

    def siblings(self, i):
        return [self.value(s, (i >> s) ^ 1) for s in range(self.depth)]

    def on_path(self, i):
        return [self.value(s, i >> s) for s in range(1, self.depth + 1)]


def check_deep(p, leaves, depth, reserve, empty):
    m = SparseModel(leaves, depth, empty)
    size = len(leaves)
    assert p.size == size and p.reserved == (reserve, held_bytes(depth, reserve))
    assert p.root() == m.root() and p.empty_nodes() == m.E
    idx = sorted({0, max(size - 1, 0)})
    assert p.path_nodes(idx) == [m.on_path(i) for i in idx]
    last = (1 << depth) - 1
    (sib,) = p.paths([last])                                     # the rightmost leaf: its top sibling is the stored node (depth - 1, 0), every other one a constant
    assert sib == m.siblings(last) and sib[:-1] == m.E[:depth - 1] and sib[-1] == m.value(depth - 1, 0)
    right = [reserve, reserve + 1, 2 * reserve + 1]              # just right of the reserve
    assert p.paths(right) == [m.siblings(i) for i in right]
    assert p.nodes(depth, reserve - 1, 3) == [m.value(0, j) for j in (reserve - 1, reserve, reserve + 1)]
    assert p.nodes(0) == [m.root()] and p.nodes(1) == [m.value(depth - 1, 0), m.E[depth - 1]]
    for i in idx + [last, reserve]:
        assert p.path_inputs([i]) == [bpg.merkle_path_inputs(i, m.siblings(i), m.root())]


@pytest.mark.parametrize("depth", [25, 32])
def test_deeper_than_the_dense_layout(ctx, leaves12, depth):
    empty, reserve = le(R.L - 2), 5
    for size in (0, 1, 5):
        leaves = list(leaves12[:size])
        p = ctx.merkle_tree(leaves, depth=depth, empty=empty, reserve=reserve)
        check_deep(p, leaves, depth, reserve, empty)
        for i in [i for i in sorted({0, size - 1}) if 0 <= i < size]:       # update reaches the occupied leaves only
            leaves[i] = le(1000 + i)
            p.update([i], [leaves[i]])
            check_deep(p, leaves, depth, reserve, empty)
        for bad in (size, reserve, (1 << depth) - 1):
            with pytest.raises(bpg.BpgError) as e:
                p.update([bad], [le(1)])
            assert e.value.status == 4
        with pytest.raises(bpg.BpgError) as e:                   # an index of 2^depth has no path
            p.paths([1 << depth])
        assert e.value.status == 4
        first = p.append(leaves12[100:102])                      # at size 5 the tree outgrows its reserve: 10
        leaves += leaves12[100:102]
        assert first == size
        check_deep(p, leaves, depth, 10 if size == 5 else reserve, empty)
        p.free()


# ---------------------------------------------------------------------------------------------------------------- the tree feeds the proofs
def path_wave(ctx, tmpl, trees, idx, tag):
    """one prove_batch_inputs wave over leaves `idx` of every tree in `trees`, the same blinding and randomness per index -> results, grouped by tree"""
    pre = state_before(G.PATH_LABEL)
    items = []
    for t in trees:
        nodes, inputs = t.path_nodes(idx), t.path_inputs(idx)
        items += [(t.nodes(t.depth, i, 1)[0], [], pre, G.blind(tag, k), rng("%s %d" % (tag, k)), 0, nodes[k], inputs[k]) for k, i in enumerate(idx)]
    ctx.profile_set(2)
    res = tmpl.prove_batch_inputs(items, commit=True)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    assert rep["k_witness_eval_batch"]["count"] == 2 and rep.get("k_witness_eval", {"count": 0})["count"] == 0      # one wave
    return [res[k * len(idx):(k + 1) * len(idx)] for k in range(len(trees))]


def path_template(ctx, tree):
    g0 = G.path_gated(ctx, 0, tree.nodes(tree.depth, 0, 1)[0], tree.paths([0])[0], tree.root(), prover_cls=bpg.Prover)
    return g0.prover.template(ctx, checkpoints=G.node_checkpoints(g0.prover))


def test_one_template_proves_leaves_of_both_layouts(leaves12):
    """depth 3, reserve 2: ONE gated MerklePath256 template, one wave over leaves of the prefix tree and of the dense tree of the same leaves - leaf 1 beside
    its sibling, and leaves 5 and 7 (empty, right of the reserve) - gives the same bytes for both, and verify_batch accepts them under the tree's inputs"""
    ctx = bpg.Context(0)
    ctx.gens_ensure(8192)
    p = ctx.merkle_tree(leaves12[:2], depth=3, empty=le(13), reserve=2)
    d = ctx.merkle_tree(leaves12[:2], depth=3, empty=le(13))
    tmpl = path_template(ctx, p)
    idx = [0, 1, 5, 7]
    from_p, from_d = path_wave(ctx, tmpl, [p, d], idx, "both")
    assert all(r[0] is not None for r in from_p) and [tuple(r) for r in from_p] == [tuple(r) for r in from_d]
    pre = state_before(G.PATH_LABEL)
    st, _ = tmpl.verify_batch([(_after_commit(pre, from_p[k][2]), from_p[k][2], from_p[k][0], None, 0, None, b"".join(x)) for k, x in enumerate(p.path_inputs(idx))])
    assert st == [0] * len(idx)
    p.update([1], [le(5)])                                                                                          # the old proofs fall with the root
    st, _ = tmpl.verify_batch([(_after_commit(pre, from_p[k][2]), from_p[k][2], from_p[k][0], None, 0, None, b"".join(x)) for k, x in enumerate(p.path_inputs(idx))])
    assert all(s != 0 for s in st)
    tmpl.free(); p.free(); d.free(); ctx.close()


# ---------------------------------------------------------------------------------------------------------------- orders on one context (child process)
def case_orders():
    """prefix build, dense build, append with regrow, a lockstep path wave, update and free on ONE context, each followed by the others; a second context's
    tree refused; a tree that outlives its context; the refusals on a live device; the census at zero"""
    ok = {}
    lib = bpg.lib()
    ctx = bpg.Context(0)
    ctx.gens_ensure(8192)
    depth, empty = 3, le(13)
    leaves = rand_scalars(b"prefix orders", 8)
    everything = lambda t: (all_levels(t), t.paths(list(range(8))), t.path_nodes(list(range(8))), t.size)
    idx = [0, 1, 4, 7]
    p = ctx.merkle_tree(leaves[:2], depth=depth, empty=empty, reserve=2)                        # prefix, then dense
    d = ctx.merkle_tree(leaves[:2], depth=depth, empty=empty)
    tmpl = path_template(ctx, p)
    ok["prefix then dense"] = everything(p) == everything(d)
    a, b = path_wave(ctx, tmpl, [p, d], idx, "o1")                                              # a wave, then appends (the prefix tree regrows: 4)
    ok["wave"] = [tuple(r) for r in a] == [tuple(r) for r in b] and all(r[0] is not None for r in a)
    ok["append with regrow"] = p.append([leaves[2]]) == d.append([leaves[2]]) == 2 and p.reserved == (4, held_bytes(depth, 4)) and everything(p) == everything(d)
    p.update([0, 2], [le(1), le(2)]); d.update([0, 2], [le(1), le(2)])                          # update after regrow, then a wave
    ok["update after regrow"] = everything(p) == everything(d)
    a, b = path_wave(ctx, tmpl, [d, p], idx, "o2")
    ok["wave after update"] = [tuple(r) for r in a] == [tuple(r) for r in b]
    q = ctx.merkle_tree(leaves[:1], depth=32, reserve=1)                                        # a deep tree beside them, free in the middle
    d.free()
    ok["append after a free"] = p.append(leaves[3:6]) == 3 and p.reserved[0] == 8 and q.append(leaves[1:3]) == 1 and q.reserved[0] == 3
    d = ctx.merkle_tree([le(1), leaves[1], le(2)] + leaves[3:6], depth=depth, empty=empty)       # dense after prefix work
    ok["dense after prefix"] = everything(p) == everything(d)
    m = SparseModel(leaves[:3], 32)
    ok["deep tree"] = q.root() == m.root() and q.paths([2, (1 << 32) - 1]) == [m.siblings(2), m.siblings((1 << 32) - 1)]
    p.free()
    p = ctx.merkle_tree([], depth=depth, empty=empty, reserve=1)                                # from nothing
    ok["from nothing"] = p.root() == empty_chain(depth, empty)[depth] and p.append(leaves[:2]) == 0 and p.reserved[0] == 2
    p.update([1], [le(3)])
    a, = path_wave(ctx, tmpl, [p], idx, "o3")
    ok["wave on a fresh tree"] = all(r[0] is not None for r in a)
    # refusals on a live device: *out is NULL, nothing is written
    h = C.c_void_p(0x5a)
    bad = []
    for dd, rr, ss, data in ((0, 1, 0, None), (33, 1, 0, None), (3, 0, 0, None), (3, 9, 1, bytes(32)), (32, (1 << 24) + 1, 1, bytes(32)), (3, 2, 3, bytes(96)), (3, 2, 1, None)):
        h.value = 0x5a
        bad.append((lib.bpg_merkle_build_prefix(ctx._h, C.c_uint32(dd), C.c_uint64(rr), C.c_uint64(ss), data, None, C.byref(h)), h.value))
    ok["build refusals"] = bad == [(4, None)] * 7
    r, by = C.c_uint64(0x5a5a), C.c_uint64(0x5a5a)
    ok["NULL handles"] = [lib.bpg_merkle_reserve(ctx._h, None, C.c_uint64(1)), lib.bpg_merkle_reserved(ctx._h, None, C.byref(r), C.byref(by)),
                          lib.bpg_merkle_reserved(ctx._h, p._h, None, None)] == [4, 4, 4] and r.value == by.value == 0x5a5a
    # a second context's prefix tree is refused here, and serves there; then it outlives its context
    other = bpg.Context(0)
    t2 = other.merkle_tree(leaves[:2], depth=25, reserve=2)
    foreign = [lib.bpg_merkle_reserve(ctx._h, t2._h, C.c_uint64(4)), lib.bpg_merkle_reserved(ctx._h, t2._h, C.byref(r), C.byref(by)),
               lib.bpg_merkle_append(ctx._h, t2._h, C.c_uint64(1), leaves[2], None, None)]
    ok["another context's tree"] = foreign == [4, 4, 4] and r.value == by.value == 0x5a5a and t2.reserved == (2, held_bytes(25, 2))
    t2.reserve(3)
    ok["its own context"] = t2.append([leaves[2]]) == 2 and t2.reserved == (3, held_bytes(25, 3)) and t2.root() == SparseModel(leaves[:3], 25).root()
    other.close()
    gone = [lib.bpg_merkle_reserve(other._h, t2._h, C.c_uint64(4)) if other._h else 4, lib.bpg_merkle_reserve(ctx._h, t2._h, C.c_uint64(4)),
            lib.bpg_merkle_reserved(ctx._h, t2._h, C.byref(r), C.byref(by))]
    ok["a tree whose context is gone"] = gone == [4, 4, 4] and r.value == by.value == 0x5a5a
    t2.free()
    ok["the others still stand"] = everything(d)[3] == 6 and q.size == 3 and p.size == 2
    tmpl.free()
    d.free()
    ctx.close()                                                                                 # over its unfreed prefix trees p and q
    p.free(); q.free()
    return {"ok": ok, "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}


def test_orders_on_one_context():
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_merkle_prefix_gpu.py"), "child"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(out["ok"].values()), out
    assert out["end"] == [0] * 6, out


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    print(json.dumps(case_orders()))
