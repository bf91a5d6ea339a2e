"""Checkpointed circuit templates on the GPU (bpg_r1cs_upload_template_checkpointed, bpg_r1cs_assign_checkpointed).

The yardstick is the EXISTING path: the host assembly of the same witness, uploaded and proved with the same transcript state, blindings and rng seed.  A
template that was handed the checkpoint values must leave exactly that witness - the proof bytes are equal - and so must a second template of the same
circuit WITHOUT checkpoints.  The checkpoint values never come from the circuit: Python integers for the chain, the native host sponge for the hash circuits
(checkpoint_cases.py), the resident tree (MerkleTree.path_nodes) in the tree-link test.

Shapes are the smallest that take every path: the 36-multiplier chain (1 level of 6 lanes), a 3-block preimage (1 level), depth-3 Merkle paths (2 levels),
and repeats of the chain with K = 5 and K = 70 (more items than the 64 lanes of a block)."""
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
import checkpoint_cases as CK

pytestmark = pytest.mark.gpu
SEED = hashlib.sha256(b"template checkpoints").digest()
MISMATCH, MISSING, INVALID = 9, 5, 4


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(8192)
    yield c
    c.close()


def host_proof(ctx, a):
    """the existing path: the host-assembled instance, uploaded and proved"""
    inst = a.prover.instance()
    res = ctx.upload(inst)
    proof, _ = res.prove(a.transcript.state, inst.v_blinding, SEED)
    res.free()
    return inst, proof


def rows_of(a):
    return getattr(a, "param_rows", None) or [CK.last_row(a)]


def params_of(a, inst):
    return [CK.constant_term(inst, r) for r in rows_of(a)]


def templates(ctx, base):
    """(checkpointed, plain): two templates of one circuit"""
    return (base.prover.template(ctx, param_rows=rows_of(base), checkpoints=base.ck_vars), base.prover.template(ctx, param_rows=rows_of(base)))


def launches(ctx, fn):
    """fn() under the all-kernels profile -> (its result, {kernel: launches})"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: v["count"] for k, v in rep.items()}


CIRCUITS = {
    "chain": (lambda ctx, seed: CK.chain(ctx, seed=seed), 1),
    "preimage3": (lambda ctx, seed: CK.preimage3(ctx, seed=seed), 1),
    "path0": (lambda ctx, seed: CK.path(ctx, 0, seed=seed), 2),
    "path5": (lambda ctx, seed: CK.path(ctx, 5, seed=seed), 2),
    "path7": (lambda ctx, seed: CK.path(ctx, 7, seed=seed), 2),
}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_checkpointed_assign_leaves_the_host_witness(ctx, name):
    build, levels = CIRCUITS[name]
    base = build(ctx, 1)
    ck, plain = templates(ctx, base)
    assert ck.n_ck == len(base.ck_vars) > 0 and plain.n_ck == 0
    try:
        for seed in (2, 3):
            a = build(ctx, seed)
            inst, want = host_proof(ctx, a)
            assert inst.v != base.prover.instance().v and a.ck_values != base.ck_values
            _, counts = launches(ctx, lambda: ck.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values))
            assert counts.get("k_witness_eval") == levels and counts.get("k_witness_ck_verify") == 1, counts
            assert set(counts) == {"k_sc_from_bytes", "k_witness_eval", "k_witness_ck_verify"}, counts
            (got, _), prove_ck = launches(ctx, lambda: ck.prove(a.transcript.state, inst.v_blinding, SEED))
            assert got == want, "%s seed %d: the checkpointed template and the host assembly give different proofs" % (name, seed)
            plain.assign(inst.v, params_of(a, inst))
            (got_plain, _), prove_plain = launches(ctx, lambda: plain.prove(a.transcript.state, inst.v_blinding, SEED))
            assert got_plain == want
            assert prove_ck == prove_plain, "a prove after a checkpointed assign launches what it launched before"
            assert ck.check().ok
            coms = b"".join(a.commitments)
            assert ck.verify(a.transcript.state, coms, got) == 0
            assert ctx.verify_flat(inst, a.transcript.state, coms, got) == 0
    finally:
        ck.free(); plain.free()


def test_mismatch_leaves_no_witness(ctx):
    base = CK.chain(ctx, seed=1)
    ck, plain = templates(ctx, base)
    try:
        a = CK.chain(ctx, seed=2)
        inst, want = host_proof(ctx, a)
        ck.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values)              # a good witness first: the mismatch must take it away
        for bad_at in ([3], [4, 1]):
            vals = list(a.ck_values)
            for k in bad_at:
                vals[k] = bpg.scalar_op("add", vals[k], bpg.scalar_from_int(1))
            with pytest.raises(bpg.BpgError) as e:
                ck.assign(inst.v, params_of(a, inst), checkpoints=vals)
            assert e.value.status == MISMATCH and e.value.first_mismatch == min(bad_at) and "checkpoint %d" % min(bad_at) in str(e.value), str(e.value)
            with pytest.raises(bpg.BpgError) as e:
                ck.prove(a.transcript.state, inst.v_blinding, SEED)
            assert e.value.status == MISSING
            with pytest.raises(bpg.BpgError) as e:
                ck.check()
            assert e.value.status == MISSING
        # x + l (below 2^255) is the same scalar
        vals = [(int.from_bytes(b, "little") + bpg.L).to_bytes(32, "little") if int.from_bytes(b, "little") + bpg.L < 1 << 255 else b for b in a.ck_values]
        assert vals != a.ck_values
        ck.assign(inst.v, params_of(a, inst), checkpoints=vals)
        assert ck.prove(a.transcript.state, inst.v_blinding, SEED)[0] == want
        # refusals on a checkpointed template, each before any work: the witness stays
        for call in (lambda: ck.assign(inst.v, params_of(a, inst)),
                     lambda: ck.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values[:-1]),
                     lambda: plain.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values),
                     lambda: ck.prove_batch([(inst.v, params_of(a, inst), a.transcript.state, inst.v_blinding, SEED, 0)]),
                     lambda: ck.prove_batch_commit([(inst.v, params_of(a, inst), a.transcript.state, inst.v_blinding, SEED, 0)])):
            with pytest.raises(bpg.BpgError) as e:
                call()
            assert e.value.status == INVALID, str(e.value)
        assert ck.prove(a.transcript.state, inst.v_blinding, SEED)[0] == want
        plain.assign(inst.v, params_of(a, inst), checkpoints=[])                    # no checkpoints, none given: plain assign
        assert plain.prove(a.transcript.state, inst.v_blinding, SEED)[0] == want
    finally:
        ck.free(); plain.free()


def test_tree_link(ctx):
    """the resident tree feeds the path template: committed values from paths(), checkpoints from path_nodes(), the parameter from root()"""
    depth, index = 3, 5
    leaves = [bpg.be_to_scalar(b) for b in CK.tree_leaves(7, 1 << depth)]
    tree = ctx.merkle_tree(leaves)
    ck = None
    try:
        nodes = tree.path_nodes(list(range(8)))
        for i in range(8):
            assert nodes[i] == [tree.nodes(depth - 1 - j, i >> (j + 1), 1)[0] for j in range(depth)], i
            assert nodes[i][-1] == tree.root()
        assert nodes == [CK.path_nodes(CK.host_tree(leaves), i) for i in range(8)]
        base = CK.path(ctx, index, depth=depth, seed=1)
        ck = base.prover.template(ctx, param_rows=[CK.last_row(base)], checkpoints=base.ck_vars)

        def prove_from_tree(leaves, old_nodes=None):
            sib = tree.paths([index])[0]
            values = [leaves[index] if what == "leaf" else sib[k] for what, k in base.order]
            a = CK.path_from(ctx, CK.host_tree(leaves), index, "ck-link")       # the host's commitments and transcript for the same values
            assert a.values == values and a.root == tree.root()
            inst = a.prover.instance()
            minus_root = bpg.scalar_op("sub", bytes(32), tree.root())
            assert minus_root == CK.constant_term(inst, CK.last_row(a))
            if old_nodes is not None:
                with pytest.raises(bpg.BpgError) as e:
                    ck.assign(values, [minus_root], checkpoints=old_nodes)
                assert e.value.status == MISMATCH
                first = e.value.first_mismatch
            else:
                first = None
            ck.assign(values, [minus_root], checkpoints=tree.path_nodes([index])[0])
            proof, _ = ck.prove(a.transcript.state, inst.v_blinding, SEED)
            assert proof == host_proof(ctx, a)[1]
            assert ck.verify(a.transcript.state, b"".join(a.commitments), proof) == 0
            return first

        assert prove_from_tree(leaves) is None
        old = tree.path_nodes([index])[0]
        leaves = list(leaves); leaves[7] = bpg.scalar_from_int(123456789)
        tree.update([7], [leaves[7]])
        # leaf 7 is under leaf 5's grandparent, not under its parent: the lowest changed ancestor is path node 1
        assert tree.path_nodes([index])[0][0] == old[0] and tree.path_nodes([index])[0][1] != old[1]
        assert prove_from_tree(leaves, old_nodes=old) == 1
    finally:
        if ck is not None:
            ck.free()
        tree.free()


@pytest.mark.parametrize("K", [5, 70])
def test_repeat(ctx, K):
    base = CK.chain(ctx, seed=1)
    ck, plain = templates(ctx, base)
    rep = rep_plain = None
    try:
        rep, rep_plain = ck.repeat(K), plain.repeat(K)
        assert rep.n_ck == 5 * K and rep_plain.n_ck == 0
        a = CK.chain(ctx, seed=2, items=K)
        inst, want = host_proof(ctx, a)
        assert (inst.n, inst.m) == (36 * K, 6 * K) == (rep.n, rep.m) and len(a.ck_values) == 5 * K
        _, counts = launches(ctx, lambda: rep.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values))
        assert counts.get("k_witness_eval_repeat") == 1 and counts.get("k_witness_ck_verify") == 1 and "k_witness_eval" not in counts, counts
        got, _ = rep.prove(a.transcript.state, inst.v_blinding, SEED)
        rep_plain.assign(inst.v, params_of(a, inst))
        assert got == rep_plain.prove(a.transcript.state, inst.v_blinding, SEED)[0] == want
        assert rep.check().ok and rep.verify(a.transcript.state, b"".join(a.commitments), got) == 0
        item, k = K - 4, 2                                                          # K = 70: item 66, past the first block of 64 items
        vals = list(a.ck_values)
        vals[5 * item + k] = bpg.scalar_op("add", vals[5 * item + k], bpg.scalar_from_int(1))
        vals[5 * (K - 1) + 4] = bytes(32)                                           # a later one as well: the lowest is reported
        with pytest.raises(bpg.BpgError) as e:
            rep.assign(inst.v, params_of(a, inst), checkpoints=vals)
        assert e.value.status == MISMATCH and e.value.first_mismatch == 5 * item + k and "item %d" % item in str(e.value), str(e.value)
        with pytest.raises(bpg.BpgError) as e:
            rep.prove(a.transcript.state, inst.v_blinding, SEED)
        assert e.value.status == MISSING
        with pytest.raises(bpg.BpgError) as e:
            rep.assign(inst.v, params_of(a, inst))
        assert e.value.status == INVALID
    finally:
        for c in (rep, rep_plain, ck, plain):
            if c is not None:
                c.free()


def test_resources_return(ctx):
    def cycle():
        base = CK.chain(ctx, seed=1)
        ck, plain = templates(ctx, base)
        rep = ck.repeat(3)
        a = CK.chain(ctx, seed=2, items=3)
        inst = a.prover.instance()
        rep.assign(inst.v, params_of(a, inst), checkpoints=a.ck_values)
        rep.prove(a.transcript.state, inst.v_blinding, SEED)
        tree = ctx.merkle_tree([bpg.scalar_from_int(i + 1) for i in range(8)])
        tree.path_nodes([0, 7])
        for c in (rep, ck, plain, tree):
            c.free()
    cycle()                                                                        # the context's own staging buffers grow once
    start = bpg.live_resources()
    cycle()
    assert bpg.live_resources() == start
