"""Growing MiMC Merkle trees on the GPU (bpg_merkle_build_partial, bpg_merkle_append, bpg_merkle_size, bpg_merkle_empty_nodes; k_merkle_fill_empty,
k_merkle_level_range and k_merkle_climb of csrc/hip/k_mimc.cuh, launched from csrc/host/merkle_plan.hpp).

The reference is the model below: pad the leaves with `empty` reduced mod l, then level by level with the oracle's sponge.  EVERY node of every level is
compared with it after every build and every append, and with the existing full build over the padded list.  The model remembers the pairs it has hashed,
so the thirteen depth-10 builds and the append sequence, which share their leaves, pay the oracle once per distinct node.

The launch log of every build and append is checked against what (depth, old size, new size) say: one fill per build and none per append, one climb
wherever a leaf is involved, one k_merkle_level_range per level whose parent range exceeds 256, exactly as many node evaluations as the new leaves have
distinct proper ancestors, and none of the full tree's kernels.

The census of live resources is process-wide and this process holds the contexts of other tests, so the scenario that ends with a census of zero runs in a
child process: this file run as `python tests/test_merkle_grow_gpu.py child` prints one JSON line."""
import ctypes as C
import functools
import hashlib
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

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
le = lambda x: x.to_bytes(32, "little")
red = lambda b: le(int.from_bytes(b, "little") % R.L)
EMPTIES = [None, le(1), le(R.L - 1), le(2**256 - 1)]           # NULL = zero; the last one is unreduced: `empty` is taken mod l, as a leaf is
NODE_PRODUCTS = 2 * 2 * 486                                   # two blocks, 486 rounds, a square and a product per round
TOP = 256                                                     # BPG_MERKLE_TOP_PARENTS: a wider parent range is one launch of its own
KERNELS = ("k_merkle_fill_empty", "k_merkle_level_range", "k_merkle_climb", "k_merkle_level", "k_merkle_top", "k_merkle_level_list")
SEED = hashlib.sha256(b"merkle grow").digest()


def rand_scalars(tag, n):
    out, i = [], 0
    while len(out) < n:
        d = hashlib.shake_256(b"%s-%d" % (tag, i)).digest(32 * 64)
        out += [le(int.from_bytes(d[32 * k:32 * k + 32], "little") % R.L) for k in range(64)]
        i += 1
    return out[:n]


# ---------------------------------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def node(left, right):
    return O.mimc_sponge(left + right)


def model(leaves, depth, empty=None):
    """levels[0] = [root] ... levels[depth] = the 2^depth leaves: the tree over leaves || empty x (2^depth - len(leaves)), everything reduced mod l"""
    level = [red(x) for x in leaves] + [red(empty or bytes(32))] * ((1 << depth) - len(leaves))
    levels = [level]
    while len(level) > 1:
        level = [node(level[i], level[i + 1]) for i in range(0, len(level), 2)]
        levels.append(level)
    return levels[::-1]


def empty_chain(depth, empty=None):
    E = [red(empty or bytes(32))]
    for _ in range(depth):
        E.append(node(E[-1], E[-1]))
    return E


def all_levels(tree):
    return [tree.nodes(level) for level in range(tree.depth + 1)]


def logged(ctx, fn):
    """fn() under the all-kernels profile -> (its result, launches, node evaluations) of the tree kernels"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    count = {k: rep.get(k, {}).get("count", 0) for k in KERNELS}
    evals = {k: rep.get(k, {}).get("field_mults", 0) / NODE_PRODUCTS for k in KERNELS}
    return res, count, evals


def check_log(count, evals, depth, old, new, build):
    """what the launch log of growing a depth-`depth` tree from `old` to `new` leaves must say"""
    ancestors = [{((1 << depth) + i) >> lv for i in range(old, new)} for lv in range(1, depth + 1)]         # per level above the leaves, as sets
    wide = sum(1 for a in ancestors if len(a) > TOP)
    assert count["k_merkle_fill_empty"] == (1 if build else 0), count
    assert count["k_merkle_climb"] == (1 if new > old else 0), count
    assert count["k_merkle_level_range"] == wide, (count, wide)
    assert evals["k_merkle_level_range"] + evals["k_merkle_climb"] == sum(len(a) for a in ancestors), (evals, sum(len(a) for a in ancestors))
    assert evals["k_merkle_fill_empty"] == 0
    assert count["k_merkle_level"] == count["k_merkle_top"] == count["k_merkle_level_list"] == 0, count


def check_build(ctx, leaves, depth, empty=None, full=True):
    """build, compare every node with the model (and with the full build over the padded list), check the launch log -> the tree"""
    t, count, evals = logged(ctx, lambda: ctx.merkle_tree(leaves, depth=depth, empty=empty))
    want = model(leaves, depth, empty)
    got = all_levels(t)
    for lv in range(depth + 1):
        assert got[lv] == want[lv], "depth %d, %d leaves: level %d differs from the model" % (depth, len(leaves), lv)
    assert t.root() == want[0][0] and t.size == len(leaves) and t.capacity == 1 << depth and t.depth == depth
    check_log(count, evals, depth, 0, len(leaves), True)
    if full:
        f = ctx.merkle_tree(want[depth])
        assert all_levels(f) == got
        f.free()
    return t


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def leaves11():
    """the leaves every depth-10 and depth-11 test takes a prefix of; nobody changes them"""
    return rand_scalars(b"grow", 1 << 11)


# ---------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_build_every_size_of_a_small_tree(ctx, depth):
    leaves = rand_scalars(b"small%d" % depth, 1 << depth)
    for size in range((1 << depth) + 1):
        check_build(ctx, leaves[:size], depth).free()


@pytest.mark.parametrize("size", [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 514, 1023, 1024])
def test_build_depth10(ctx, leaves11, size):
    """both sides of the 256-parent hand-over (513 leaves are 257 parents: one wide step) and of the block edges"""
    check_build(ctx, leaves11[:size], 10).free()


def test_build_depth11_two_wide_steps(ctx, leaves11):
    """1,539 leaves: 770 parents at level 10 (three full blocks and two lanes), 385 at level 9, then the climb"""
    t, count, evals = logged(ctx, lambda: ctx.merkle_tree(leaves11[:1539], depth=11))
    assert all_levels(t) == model(leaves11[:1539], 11)
    check_log(count, evals, 11, 0, 1539, True)
    assert count["k_merkle_level_range"] == 2 and evals["k_merkle_level_range"] == 770 + 385
    t.free()


def test_no_leaf_no_hashing(ctx):
    t, count, evals = logged(ctx, lambda: ctx.merkle_tree([], depth=10, empty=le(5)))
    assert count["k_merkle_fill_empty"] == 1 and sum(count.values()) == 1 and sum(evals.values()) == 0
    assert t.root() == empty_chain(10, le(5))[10] and t.size == 0
    t.free()


# ---------------------------------------------------------------------------------------------------------------- the empty value
@pytest.mark.parametrize("which", range(4))
def test_empty_values(ctx, which):
    empty, depth = EMPTIES[which], 5
    leaves = rand_scalars(b"empty%d" % which, 5)
    leaves[3] = le(2**256 - 1)                                               # an unreduced leaf reads back reduced
    t = check_build(ctx, leaves, depth, empty)
    E = empty_chain(depth, empty)
    assert t.empty_nodes() == E and E[0] == red(empty or bytes(32))
    assert t.nodes(depth, 3, 1) == [le((2**256 - 1) % R.L)]
    for lv in range(depth + 1):                                              # level depth - lv holds E[lv] from its first node without a leaf on
        first = -(-5 // (1 << lv))
        got = t.nodes(depth - lv, first)
        assert got == [E[lv]] * ((1 << (depth - lv)) - first), lv
    t.free()


def test_empty_nodes_of_a_full_tree(ctx):
    """a tree of bpg_merkle_build has empty = 0 and computes the table at the first call"""
    t = ctx.merkle_tree(rand_scalars(b"full", 16))
    assert t.size == 16 == t.capacity
    assert t.empty_nodes() == empty_chain(4) == t.empty_nodes()
    t.free()


# ---------------------------------------------------------------------------------------------------------------- append
def check_append(ctx, t, have, new, depth, empty=None):
    """append `new` to a tree holding `have`, compare outputs, every node and the launch log -> the leaves it holds now"""
    (first, root), count, evals = logged(ctx, lambda: t.append(new, return_root=True))
    now = have + list(new)
    want = model(now, depth, empty)
    assert first == len(have) and root == want[0][0] == t.root() and t.size == len(now)
    got = all_levels(t)
    for lv in range(depth + 1):
        assert got[lv] == want[lv], "depth %d, %d -> %d leaves: level %d differs from the model" % (depth, len(have), len(now), lv)
    check_log(count, evals, depth, len(have), len(now), False)
    return now


def test_append_sequence(ctx, leaves11):
    """from nothing to full at depth 10: 1, 1, 2, 252 (-> 256), 1 (-> 257), 254, 1 (an odd start beside an old left sibling), then the rest"""
    depth, empty = 10, le(9)
    t = check_build(ctx, [], depth, empty, full=False)
    have, at = [], 0
    for k in (1, 1, 2, 252, 1, 254, 1):
        have = check_append(ctx, t, have, leaves11[at:at + k], depth, empty); at += k
    assert at == 512
    have = check_append(ctx, t, have, leaves11[at:1 << depth], depth, empty)                          # the whole right half: 256 parents, no wide step
    assert t.size == t.capacity == len(have)
    f = ctx.merkle_tree(have)
    assert all_levels(f) == all_levels(t)
    f.free()
    # full now: nothing more goes in, and an empty append still answers
    before = all_levels(t)
    with pytest.raises(bpg.BpgError) as e:
        t.append([le(1)])
    assert e.value.status == 4 and t.size == 1 << depth
    assert t.append([], return_root=True) == (1 << depth, before[0][0])
    assert all_levels(t) == before
    t.free()


def test_append_wide(ctx, leaves11):
    """depth 11 from 3 leaves, one append of 1,536: wide steps at two levels (769 and 385 parents), the first parent shared with old leaf 2"""
    t = check_build(ctx, leaves11[:3], 11, full=False)
    have = check_append(ctx, t, leaves11[:3], leaves11[3:1539], 11)
    assert len(have) == 1539
    t.free()


def test_append_refusals(ctx, leaves11):
    depth = 4
    lib = bpg.lib()
    t = ctx.merkle_tree(leaves11[:13], depth=depth)
    before = all_levels(t)
    (first, root), count, evals = logged(ctx, lambda: t.append([], return_root=True))               # nothing to do: the outputs, no launch
    assert (first, root) == (13, before[0][0]) and t.append(b"") == 13
    assert sum(count.values()) == 0
    with pytest.raises(bpg.BpgError) as e:                                                          # 13 + 4 > 16
        t.append(leaves11[:4])
    assert e.value.status == 4
    first, out = C.c_uint64(0x5a5a), C.create_string_buffer(b"\x5a" * 32, 32)
    assert lib.bpg_merkle_append(ctx._h, t._h, C.c_uint64(4), b"".join(leaves11[:4]), C.byref(first), out) == 4
    assert lib.bpg_merkle_append(ctx._h, t._h, C.c_uint64(1), None, C.byref(first), out) == 4       # NULL leaves with a count
    assert lib.bpg_merkle_append(ctx._h, None, C.c_uint64(1), leaves11[0], C.byref(first), out) == 4
    assert lib.bpg_merkle_size(ctx._h, t._h, None, None) == 4
    assert lib.bpg_merkle_empty_nodes(ctx._h, t._h, None) == 4
    assert first.value == 0x5a5a and out.raw == b"\x5a" * 32
    assert t.size == 13 and all_levels(t) == before
    assert t.append(leaves11[13:16]) == 13 and t.size == 16                                          # exactly the room there is
    assert all_levels(t) == model(leaves11[:16], depth)
    t.free()
    # a tree of bpg_merkle_build is full
    f = ctx.merkle_tree(leaves11[:8])
    before = all_levels(f)
    with pytest.raises(bpg.BpgError) as e:
        f.append([le(1)])
    assert e.value.status == 4 and f.size == 8 and all_levels(f) == before
    assert f.append([]) == 8
    f.free()
    # what build_partial refuses on a live context: *out is NULL afterwards
    h = C.c_void_p(0x5a)
    for d, size, data in ((0, 0, None), (25, 1, bytes(32)), (2, 5, bytes(160)), (2, 1, None)):
        h.value = 0x5a
        assert lib.bpg_merkle_build_partial(ctx._h, C.c_uint32(d), C.c_uint64(size), data, None, C.byref(h)) == 4
        assert not h.value
    assert lib.bpg_merkle_build_partial(ctx._h, C.c_uint32(2), C.c_uint64(1), bytes(32), None, None) == 4
    with pytest.raises(bpg.BpgError) as e:
        ctx.merkle_tree(leaves11[:5], depth=2)
    assert e.value.status == 4
    with pytest.raises(ValueError):                                                                  # without depth: today's rule
        ctx.merkle_tree(leaves11[:3])


def test_full_build_and_update_keep_their_launches(ctx, leaves11):
    t, count, evals = logged(ctx, lambda: ctx.merkle_tree(leaves11[:1024]))
    assert (count["k_merkle_level"], count["k_merkle_top"]) == (1, 1) and evals["k_merkle_level"] == 512 and evals["k_merkle_top"] == 511
    assert count["k_merkle_fill_empty"] == count["k_merkle_level_range"] == count["k_merkle_climb"] == count["k_merkle_level_list"] == 0
    _, count, evals = logged(ctx, lambda: t.update([5, 700], [le(1), le(2)]))
    assert count["k_merkle_level_list"] == 10 and evals["k_merkle_level_list"] == 19                 # two paths that meet at the root
    assert sum(count.values()) == 10
    t.free()


# ---------------------------------------------------------------------------------------------------------------- update on a grown tree
def test_update_on_a_grown_tree(ctx, leaves11):
    depth, size, empty = 10, 300, le(3)
    leaves = list(leaves11[:size])
    t = ctx.merkle_tree(leaves, depth=depth, empty=empty)
    idx = [0, 1, 255, 256, 299]
    new = rand_scalars(b"upd", len(idx))
    _, count, evals = logged(ctx, lambda: t.update(idx, new))
    assert count["k_merkle_level_list"] == depth and count["k_merkle_climb"] == count["k_merkle_level_range"] == 0
    for i, x in zip(idx, new):
        leaves[i] = x
    want = model(leaves, depth, empty)
    assert all_levels(t) == want and t.size == size
    for bad in ([size], [size + 1], [(1 << depth) - 1], [0, size], [1 << depth]):                   # the first free slot, the empty region, beyond
        with pytest.raises(bpg.BpgError) as e:
            t.update(bad, rand_scalars(b"bad", len(bad)))
        assert e.value.status == 4
    assert all_levels(t) == want and t.size == size
    assert t.append([le(7)]) == size                                                                 # the slot opens with the leaf ...
    t.update([size], [le(8)])                                                                        # ... and then update reaches it
    assert all_levels(t) == model(leaves + [le(8)], depth, empty)
    t.free()


# ---------------------------------------------------------------------------------------------------------------- paths
def fold(leaf, index, siblings):
    h = leaf
    for lv, sib in enumerate(siblings):
        h = O.mimc_sponge(sib + h) if (index >> lv) & 1 else O.mimc_sponge(h + sib)
    return h


@pytest.mark.parametrize("which", [0, 3])
def test_paths_of_a_size5_depth3_tree(ctx, which):
    empty = EMPTIES[which]
    leaves = rand_scalars(b"paths", 5)
    t = ctx.merkle_tree(leaves, depth=3, empty=empty)
    E, want = t.empty_nodes(), model(leaves, 3, empty)
    assert E == empty_chain(3, empty)
    paths, on_path = t.paths(list(range(8))), t.path_nodes(list(range(8)))
    for i in range(8):
        assert paths[i] == [want[3 - lv][(i >> lv) ^ 1] for lv in range(3)]
        assert on_path[i] == [want[3 - lv][i >> lv] for lv in range(1, 4)]
        assert fold(want[3][i], i, paths[i]) == t.root() == on_path[i][-1]
    # a sibling is the constant E[lv] exactly when it lies in the empty region: node j of height lv holds no leaf when j >= ceil(5 / 2^lv)
    assert paths[4][0] == E[0] and paths[4][1] == E[1] and paths[4][2] == want[1][0]
    for i in range(8):
        for lv in range(3):
            assert (paths[i][lv] == E[lv]) == (((i >> lv) ^ 1) >= -(-5 // (1 << lv))), (i, lv)
    assert sum(p[lv] == E[lv] for p in paths for lv in range(3)) == 3 + 2                           # E_0 beside leaves 4, 6 and 7; E_1 above leaves 4 and 5
    t.free()


# ---------------------------------------------------------------------------------------------------------------- the tree feeds the proofs
def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def path_witnesses(leaf, index, siblings):
    pattern, witnesses = "W", [leaf]
    for lv, sib in enumerate(siblings):                      # the index bit says on which side the sibling stands
        if (index >> lv) & 1:
            pattern, witnesses = "(W %s)" % pattern, [sib] + witnesses
        else:
            pattern, witnesses = "(%s W)" % pattern, witnesses + [sib]
    return pattern, witnesses


def make_proof(ctx, root, witnesses, pattern, capacity):
    tp = bpg.Transcript(b"MerkleTree")
    p = bpg.Prover(ctx, tp)
    blind = rand_scalars(b"blind", len(witnesses))
    coms, vars_ = zip(*[p.commit(w, b) for w, b in zip(witnesses, blind)])
    bpg.MerkleTree256(root, [], bpg.vars_to_lc(vars_), pattern).prove(p, [], [])
    return list(coms), p.prove(bpg.BulletproofGens(ctx, capacity), bytes(range(32)))


def accepted(ctx, root, coms, pattern, proof, capacity):
    """(the GPU verifier's answer, the oracle verifier's) for the statement `the committed path leads to root`"""
    tv = bpg.Transcript(b"MerkleTree")
    v = bpg.Verifier(tv)
    bpg.MerkleTree256(root, [], bpg.vars_to_lc(bpg.verifier_commit(v, list(coms))), pattern).verify(v, [], [])
    vi = v.instance()
    by_oracle = O.verify(O.Gens(capacity), tv.state, to_oracle(vi), vi.commitments, proof) == 0      # first: the GPU verifier moves the transcript on
    return v.is_valid(proof, ctx, capacity), by_oracle


def test_path_proof_of_leaf4(ctx):
    """leaf 4 of a size-5, depth-3 tree: its sibling is E_0 and its uncle is E_1.  The proof stands against root(), falls with the next append, and a proof
    over the new siblings stands against the new root."""
    cap = 1 << 13
    leaves = rand_scalars(b"proof5", 6)
    t = ctx.merkle_tree(leaves[:5], depth=3, empty=le(11))
    E = t.empty_nodes()
    root, (sib,) = t.root(), t.paths([4])
    assert sib[0] == E[0] == le(11) and sib[1] == E[1]
    pattern, wit = path_witnesses(leaves[4], 4, sib)
    assert pattern == "(W ((W W) W))"
    coms, proof = make_proof(ctx, root, wit, pattern, cap)
    assert accepted(ctx, root, coms, pattern, proof, cap) == (True, True)
    first, new_root = t.append([leaves[5]], return_root=True)
    assert first == 5 and new_root == t.root() != root
    assert accepted(ctx, new_root, coms, pattern, proof, cap) == (False, False)                      # the old proof under the new root
    (sib2,) = t.paths([4])
    assert sib2[0] == leaves[5] and sib2[1] == E[1] and sib2[2] == sib[2]
    pattern2, wit2 = path_witnesses(leaves[4], 4, sib2)
    coms2, proof2 = make_proof(ctx, new_root, wit2, pattern2, cap)
    assert pattern2 == pattern and accepted(ctx, new_root, coms2, pattern2, proof2, cap) == (True, True)
    t.free()


# ---------------------------------------------------------------------------------------------------------------- orders on one context (child process)
def case_orders():
    """grown tree -> lockstep path proofs for every occupied leaf, fed from the tree -> append -> the same for six leaves; a second context's tree refused;
    the context closed before its tree is freed; the census at zero.  A path's pattern depends on the leaf index (on which side each sibling stands), so
    there is one depth-3 template per leaf and each batch call of prove_batch_checkpointed carries that template's item."""
    import checkpoint_cases as CK
    ok = {}
    lib = bpg.lib()
    ctx = bpg.Context(0)
    ctx.gens_ensure(8192)
    depth, empty = 3, le(13)
    leaves = rand_scalars(b"orders", 6)
    tree = ctx.merkle_tree(leaves[:5], depth=depth, empty=empty)
    templates = {}

    def round_of(size, tag):
        want = model(leaves[:size], depth, empty)
        good = tree.size == size and all_levels(tree) == want
        root = tree.root()
        paths, on_path = tree.paths(list(range(size))), tree.path_nodes(list(range(size)))
        for i in range(size):
            a = CK.path_from(ctx, want[::-1], i, "grow-%s-%d" % (tag, i))                       # the host's commitments and transcript for the same values
            values = [tree.nodes(depth, i, 1)[0] if what == "leaf" else paths[i][k] for what, k in a.order]
            inst = a.prover.instance()
            good &= b"".join(values) == bytes(inst.v) and a.root == root and a.ck_values == on_path[i]
            if i not in templates:
                templates[i] = a.prover.template(ctx, param_rows=[CK.last_row(a)], checkpoints=a.ck_vars)
            tmpl = templates[i]
            param = bpg.scalar_op("sub", bytes(32), root)
            post, coms = a.transcript.state, b"".join(a.commitments)
            got = tmpl.prove_batch_checkpointed([(b"".join(values), [param], post, inst.v_blinding, SEED, 0, on_path[i])])
            tmpl.assign(b"".join(values), [param], checkpoints=on_path[i])                      # the item alone
            alone = tmpl.prove(post, inst.v_blinding, SEED)
            good &= len(got) == 1 and tuple(got[0]) == tuple(alone)
            good &= tmpl.verify(post, coms, alone[0]) == 0 and ctx.verify_flat(inst, post, coms, alone[0]) == 0
        return bool(good)

    ok["five leaves"] = round_of(5, "a")
    ok["append"] = tree.append([leaves[5]], return_root=True) == (5, model(leaves[:6], depth, empty)[0][0])
    ok["six leaves"] = round_of(6, "b")
    # a second context's grown tree is refused here, and serves there
    other = bpg.Context(0)
    t2 = other.merkle_tree(leaves[:2], depth=depth)
    first, size, out = C.c_uint64(0x5a5a), C.c_uint64(0x5a5a), C.create_string_buffer(b"\x5a" * 128, 128)
    refused = [lib.bpg_merkle_append(ctx._h, t2._h, C.c_uint64(1), leaves[2], C.byref(first), out), lib.bpg_merkle_size(ctx._h, t2._h, C.byref(size), None),
               lib.bpg_merkle_empty_nodes(ctx._h, t2._h, out)]
    ok["another context's tree"] = refused == [4, 4, 4] and first.value == size.value == 0x5a5a and out.raw == b"\x5a" * 128
    ok["its own context"] = t2.append([leaves[2]]) == 2 and all_levels(t2) == model(leaves[:3], depth)
    # close the context, then free the tree: the handle is good for free() alone
    other.close()
    gone = [lib.bpg_merkle_append(ctx._h, t2._h, C.c_uint64(1), leaves[3], C.byref(first), out), lib.bpg_merkle_size(ctx._h, t2._h, C.byref(size), None),
            lib.bpg_merkle_empty_nodes(ctx._h, t2._h, out)]
    ok["a tree whose context is gone"] = gone == [4, 4, 4] and first.value == size.value == 0x5a5a and out.raw == b"\x5a" * 128
    t2.free()
    ok["the first tree still stands"] = all_levels(tree) == model(leaves[:6], depth, empty)
    for tmpl in templates.values():
        tmpl.free()
    ctx.close()                                                                                 # over its unfreed tree
    tree.free()
    return {"ok": ok, "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}


def test_orders_on_one_context():
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_merkle_grow_gpu.py"), "child"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(out["ok"].values()), out
    assert out["end"] == [0] * 6, out


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    print(json.dumps(case_orders()))
