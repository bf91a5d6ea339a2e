"""MiMC sponges and Merkle trees on the GPU (csrc/hip/k_mimc.cuh behind bpg_mimc_sponge_many and bpg_merkle_*): every digest, node, sibling and root is
compared byte for byte with the oracle's sponge, and a tree built here feeds the MerkleTree256 proofs both verifiers accept."""
import ctypes as C
import hashlib
import random
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
H = bytes.fromhex
le = lambda x: x.to_bytes(32, "little")
EDGES = [le(0), le(1), le(R.L - 1), le(2**256 - 1)]      # the last one is unreduced: a block is taken mod l
NODE_PRODUCTS = 2 * 2 * 486                             # two blocks, 486 rounds, a square and a product per round


def rand_scalars(tag, n):
    out, i = [], 0
    while len(out) < n:
        d = hashlib.shake_256(b"%s-%d" % (tag, i)).digest(32 * 64)
        out += [le(int.from_bytes(d[32 * k:32 * k + 32], "little") % R.L) for k in range(64)]
        i += 1
    return out[:n]


@pytest.fixture(scope="module")
def ctx():
    return bpg.Context(0)


def all_levels(tree):
    return [tree.nodes(level) for level in range(tree.depth + 1)]


def check_levels(levels, leaves):
    """every node is the oracle's sponge of its two children as read back; the bottom level is the leaves (canonical)"""
    assert levels[-1] == leaves
    for level in range(len(levels) - 1):
        kids = levels[level + 1]
        assert len(levels[level]) == 1 << level
        for j, node in enumerate(levels[level]):
            assert node == O.mimc_sponge(kids[2 * j] + kids[2 * j + 1]), (level, j)


def launches(ctx):
    rep = ctx.profile_report()
    count = {k: rep.get(k, {}).get("count", 0) for k in ("k_merkle_level", "k_merkle_top", "k_merkle_level_list")}
    evals = {k: rep.get(k, {}).get("field_mults", 0) / NODE_PRODUCTS for k in count}
    return count, evals


# ---------------------------------------------------------------------------------------------------------------- sponges
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_mimc_sponge_many(ctx, count, blocks):
    items = [rand_scalars(b"sp%d-%d-%d" % (count, blocks, i), blocks) for i in range(count)]
    # the edge values in the first and the last item (0, 1, l - 1 and the unreduced 2^256 - 1 all occur at each block count over the five counts)
    items[0] = [EDGES[(count + b) % 4] for b in range(blocks)]
    items[count - 1] = [EDGES[(count + b + 2) % 4] for b in range(blocks)]
    got = ctx.mimc_sponge_many(items, blocks)
    assert len(got) == count
    for i, it in enumerate(items):
        assert got[i] == O.mimc_sponge(b"".join(it)), i
    assert ctx.mimc_sponge_many(b"".join(b"".join(it) for it in items), blocks) == got


def test_mimc_sponge_many_refusals(ctx):
    lib = bpg.lib()
    out = C.create_string_buffer(b"\x5a" * 32, 32)
    assert lib.bpg_mimc_sponge_many(ctx._h, C.c_uint64(0), C.c_uint64(2), bytes(64), out) == 4
    assert lib.bpg_mimc_sponge_many(ctx._h, C.c_uint64(2), C.c_uint64(0), bytes(64), out) == 4
    assert lib.bpg_mimc_sponge_many(ctx._h, C.c_uint64(1), C.c_uint64(1), None, out) == 4
    assert lib.bpg_mimc_sponge_many(ctx._h, C.c_uint64(1), C.c_uint64(1), bytes(32), None) == 4
    assert out.raw == b"\x5a" * 32


# ---------------------------------------------------------------------------------------------------------------- trees
@pytest.fixture(scope="module")
def tree10(ctx):
    """the depth-10 tree the path and update tests share: (leaves, every level as built); nobody changes it"""
    leaves = rand_scalars(b"tree10", 1 << 10)
    t = ctx.merkle_tree(leaves)
    levels = all_levels(t)
    t.free()
    return leaves, levels


@pytest.mark.parametrize("depth", [1, 2, 3, 8, 9, 10])
def test_tree_every_node(ctx, depth):
    leaves = rand_scalars(b"tree%d" % depth, 1 << depth)
    ctx.profile_set(2)
    t = ctx.merkle_tree(leaves)
    count, evals = launches(ctx)
    ctx.profile_set(0)
    assert t.depth == depth
    levels = all_levels(t)
    check_levels(levels, leaves)
    assert t.root() == levels[0][0] == t.nodes(0, 0, 1)[0]
    assert t.nodes(depth, 1, 1) == [leaves[1]] and t.nodes(depth - 1, (1 << (depth - 1)) - 1, 1) == [levels[depth - 1][-1]]
    # the launch log: the levels below the hand-over one launch each, the rest in ONE launch, every node evaluated once
    by_level = count["k_merkle_level"]
    assert count["k_merkle_top"] == 1 and count["k_merkle_level_list"] == 0 and by_level < depth
    assert evals["k_merkle_level"] == sum(1 << lv for lv in range(depth - by_level, depth))
    assert evals["k_merkle_top"] == (1 << (depth - by_level)) - 1
    t.free()


def test_tree_depths_cross_the_hand_over(ctx):
    """depths 8, 9 and 10 straddle the hand-over between k_merkle_level and k_merkle_top, as the launch log itself shows: the shallowest takes no
    per-level launch, the deepest does, and one more level of depth is at most one more per-level launch"""
    by_level = {}
    for depth in (8, 9, 10):
        ctx.profile_set(2)
        t = ctx.merkle_tree(rand_scalars(b"cross", 1 << depth))
        by_level[depth] = launches(ctx)[0]["k_merkle_level"]
        ctx.profile_set(0)
        t.free()
    assert by_level[8] == 0 and by_level[10] > 0
    assert 0 <= by_level[9] - by_level[8] <= 1 and 0 <= by_level[10] - by_level[9] <= 1


def test_reference_tree_of_equal_leaves(ctx, golden):
    m = golden["mimc"]
    leaf = bytes(reversed(H(m["leaf512_be"])))
    t = ctx.merkle_tree([leaf] * 512)
    levels = all_levels(t)
    t.free()
    for k, want in enumerate(m["levels512_be"]):             # levels512_be[k] is k + 1 levels above the leaves (merkle_tree_gadget.rs:476-503)
        level = levels[9 - (k + 1)]
        assert bytes(reversed(level[0])).hex() == want
        assert all(x == level[0] for x in level)


def fold(leaf, index, siblings):
    h = leaf
    for lv, sib in enumerate(siblings):
        h = O.mimc_sponge(sib + h) if (index >> lv) & 1 else O.mimc_sponge(h + sib)
    return h


def test_paths(ctx, tree10):
    leaves, levels = tree10
    t = ctx.merkle_tree(leaves)
    rnd = random.Random(10)
    indices = [0, 1, (1 << 10) - 1, 1 << 9] + [rnd.randrange(1 << 10) for _ in range(20)] + [77, 77]
    for batch in ([indices[2]], indices, (indices * 3)[:65]):              # a batch of 1, one of 26, one of 65 (more than a wave of items)
        paths = t.paths(batch)
        assert len(paths) == len(batch)
        for i, p in zip(batch, paths):
            assert len(p) == 10
            assert p == [levels[10 - lv][(i >> lv) ^ 1] for lv in range(10)]
            assert fold(leaves[i], i, p) == levels[0][0]
    assert t.paths([]) == []
    with pytest.raises(bpg.BpgError) as e:
        t.paths([0, 1 << 10])
    assert e.value.status == 4
    t.free()


def test_updates(ctx, tree10):
    leaves, levels = tree10
    leaves = list(leaves)
    t = ctx.merkle_tree(leaves)
    rnd = random.Random(5)
    for k, idx in enumerate([[0], [0, 1], [(1 << 10) - 1], rnd.sample(range(1 << 10), 100)]):
        new = rand_scalars(b"upd%d" % k, len(idx))
        if k == 3:
            new[0] = EDGES[3]                                               # an unreduced leaf reads back reduced
        ctx.profile_set(2)
        t.update(idx, new)
        count, evals = launches(ctx)
        ctx.profile_set(0)
        for i, x in zip(idx, new):
            leaves[i] = le(int.from_bytes(x, "little") % R.L)
        fresh = ctx.merkle_tree(leaves)
        assert all_levels(t) == all_levels(fresh)
        fresh.free()
        # only the ancestors: one launch per level, and as many node evaluations as there are distinct ancestors
        want = sum(len({((1 << 10) + i) >> lv for i in idx}) for lv in range(1, 11))
        assert count["k_merkle_level_list"] == 10 and count["k_merkle_level"] == 0 and count["k_merkle_top"] == 0
        assert evals["k_merkle_level_list"] == want
        if k < 3:
            assert want == 10                                               # one leaf, or two under one parent: `depth` evaluations, not 2^depth
    check_levels(all_levels(t), leaves)
    before = all_levels(t)
    for bad_idx in ([3, 9, 3], [1 << 10], [0, 2**40]):                       # a duplicate, out of range
        with pytest.raises(bpg.BpgError) as e:
            t.update(bad_idx, rand_scalars(b"bad", len(bad_idx)))
        assert e.value.status == 4
    assert bpg.lib().bpg_merkle_update(ctx._h, t._h, C.c_uint64(1), None, bytes(32)) == 4
    assert all_levels(t) == before
    t.free()
    with pytest.raises(ValueError):
        t.root()


def test_build_refusals(ctx):
    lib = bpg.lib()
    h = C.c_void_p(0x5a)
    for depth in (0, 25):
        assert lib.bpg_merkle_build(ctx._h, C.c_uint32(depth), bytes(64), C.byref(h)) == 4
        assert not h.value
    assert lib.bpg_merkle_build(ctx._h, C.c_uint32(1), None, C.byref(h)) == 4
    assert lib.bpg_merkle_build(ctx._h, C.c_uint32(1), bytes(64), None) == 4
    t = ctx.merkle_tree([le(1), le(2)])
    out = C.create_string_buffer(b"\x5a" * 64, 64)
    assert lib.bpg_merkle_nodes(ctx._h, t._h, C.c_uint32(2), C.c_uint64(0), C.c_uint64(1), out) == 4       # a level above the depth
    assert lib.bpg_merkle_nodes(ctx._h, t._h, C.c_uint32(1), C.c_uint64(1), C.c_uint64(2), out) == 4       # beyond the level
    assert lib.bpg_merkle_nodes(ctx._h, t._h, C.c_uint32(1), C.c_uint64(0), C.c_uint64(2), None) == 4
    assert lib.bpg_merkle_root(ctx._h, t._h, None) == 4
    assert out.raw == b"\x5a" * 64
    assert t.root() == O.mimc_sponge(le(1) + le(2))
    t.free()
    with pytest.raises(ValueError):
        ctx.merkle_tree([le(1)] * 3)


# ---------------------------------------------------------------------------------------------------------------- the tree feeds the proofs
def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def prove_and_verify(ctx, root, witnesses, pattern, capacity, expect_ok):
    """MerkleTree256 over committed leaves with `root` as the constant: Prover.prove on the GPU, then the GPU verifier and the oracle's"""
    tp = bpg.Transcript(b"MerkleTree")
    p = bpg.Prover(ctx, tp)
    blind = rand_scalars(b"blind", len(witnesses))
    coms, vars_ = zip(*[p.commit(w, b) for w, b in zip(witnesses, blind)])
    bpg.MerkleTree256(root, [], bpg.vars_to_lc(vars_), pattern).prove(p, [], [])
    inst = p.instance()
    assert O.satisfied(to_oracle(inst), inst.v) == expect_ok
    proof = p.prove(bpg.BulletproofGens(ctx, capacity), bytes(range(32)))
    tv = bpg.Transcript(b"MerkleTree")
    v = bpg.Verifier(tv)
    bpg.MerkleTree256(root, [], bpg.vars_to_lc(bpg.verifier_commit(v, list(coms))), pattern).verify(v, [], [])
    vi = v.instance()
    assert (O.verify(O.Gens(capacity), tv.state, to_oracle(vi), vi.commitments, proof) == 0) == expect_ok
    assert v.is_valid(proof, ctx, capacity) == expect_ok


def test_full_tree_root_is_the_circuits_constant(ctx):
    leaves = rand_scalars(b"full8", 8)
    t = ctx.merkle_tree(leaves)
    root = t.root()
    pattern = "(((W W) (W W)) ((W W) (W W)))"
    prove_and_verify(ctx, root, leaves, pattern, 1 << 14, True)
    t.update([6], rand_scalars(b"other", 1))
    other = t.root()
    t.free()
    assert other != root
    prove_and_verify(ctx, other, leaves, pattern, 1 << 14, False)


def test_depth3_path_proof(ctx):
    leaves = rand_scalars(b"path8", 8)
    t = ctx.merkle_tree(leaves)
    root, (siblings,) = t.root(), t.paths([5])
    t.free()
    pattern, witnesses = "W", [leaves[5]]
    for lv, sib in enumerate(siblings):                      # the index bit says on which side the sibling stands
        if (5 >> lv) & 1:
            pattern, witnesses = "(W %s)" % pattern, [sib] + witnesses
        else:
            pattern, witnesses = "(%s W)" % pattern, witnesses + [sib]
    assert pattern == "(W ((W W) W))"
    prove_and_verify(ctx, root, witnesses, pattern, 1 << 13, True)


# ---------------------------------------------------------------------------------------------------------------- two contexts
def test_two_contexts_and_free(ctx):
    leaves = rand_scalars(b"two", 1 << 6)
    t = ctx.merkle_tree(leaves)
    root = t.root()
    other = bpg.Context(0)
    t2 = other.merkle_tree(rand_scalars(b"two-b", 1 << 6))
    assert t2.root() != root
    with pytest.raises(bpg.BpgError) as e:                   # a tree belongs to its context
        out = C.create_string_buffer(32)
        bpg._chk(bpg.lib().bpg_merkle_root(ctx._h, t2._h, out))
    assert e.value.status == 4
    t2.update([3], [le(7)])
    t2.free()
    # a context that goes before its tree takes the tree's memory with it: the handle is good for free() alone, whichever way it is freed
    t3, t4 = other.merkle_tree(leaves), other.merkle_tree(leaves)
    other.close()
    out = C.create_string_buffer(32)
    assert bpg.lib().bpg_merkle_root(ctx._h, t3._h, out) == 4
    bpg.lib().bpg_merkle_free(ctx._h, t3._h)                  # through another context
    t3._h = None
    t4.free()                                                # through none
    check_levels(all_levels(t), leaves)
    assert t.root() == root
    t.free()
    # freeing returns the memory: a tree of 2^20 leaves (64 MB) twice in a row, the second where the first was
    big = hashlib.shake_256(b"big").digest(32 << 20)
    big = b"".join(big[i:i + 31] + b"\x0f" for i in range(0, len(big), 32))             # below 2^252: canonical
    roots = []
    for _ in range(2):
        tb = ctx.merkle_tree(big)
        assert tb.depth == 20 and tb.nodes(20, (1 << 20) - 1, 1) == [big[-32:]]
        roots.append(tb.root())
        tb.free()
    assert roots[0] == roots[1]
    kids = ctx.merkle_tree(big[:64])
    assert kids.root() == O.mimc_sponge(big[:64])
    kids.free()
