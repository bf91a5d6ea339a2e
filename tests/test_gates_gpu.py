"""Gated variables on the GPU (bpg_r1cs_upload_template_gated, k_witness_eval / k_witness_eval_batch reading gated terms, k_vw_flatten reading an item's
coefficient tail): ONE template serves every input vector of the hand-made circuit and every leaf index of a resident Merkle tree.

The yardstick is never the template: proofs are compared byte for byte with the CPU oracle's proof of a FRESH HOST ASSEMBLY that knows nothing of inputs or
gates (gate_cases.py: hand10(gated=False); for paths the reference gadget MerkleTree256 over the index's own pattern with the siblings baked in), and judged
by verifiers assembled from that reference circuit.

Run as a script (`python tests/test_gates_gpu.py child`) the file runs the grown-tree scenario in a process of its own, frees everything and prints the
census of what the process still holds (bpg_test_live_resources)."""
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
import gate_cases as G
from gate_cases import sc, L
from template_inputs_cases import rng

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
MISMATCH = bpg.ERR_CHECKPOINT_MISMATCH
LC = bpg.LinearCombination


def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def state_before(label):
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(label)
    bpg.Prover(None, t)
    return t.state


class Ref:
    """the yardstick of one statement: the reference assembly (no inputs, no gates), its transcript after the commitments, and the oracle's proof of it"""
    def __init__(self, case, tag, gens=None):
        self.case, self.tag = case, tag
        self.inst = case.prover.instance()
        self.state, self.coms = case.transcript.state, b"".join(case.commitments)
        self.proof = self.state_after = None
        if gens is not None:
            rc, self.proof, self.state_after = O.prove(gens, self.state, to_oracle(self.inst), self.inst.v_blinding, rng(tag), O.FLAG_FAST_MSM)
            assert rc == 0


def reference_verdict(ctx, index, com, siblings, root, proof, cap):
    """a verifier assembled from the REFERENCE gadget for this index, these siblings and this root judges the proof on the GPU"""
    v = bpg.Verifier(bpg.Transcript(G.PATH_LABEL))
    var = v.commit(com)
    pat, order = G.reference_pattern(index, len(siblings))
    bpg.MerkleTree256(root, [siblings[k] for k in order], [LC.of(var)], pat).verify(v, [], [])
    return v.is_valid(proof, ctx, cap)


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(4096)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. the hand-made circuit, N = 16
@pytest.fixture(scope="module")
def hand(ctx):
    gens = O.Gens(16)
    tmpl = G.hand10(G.HAND_INPUTS[0], G.HAND_VALUES[0], True, prover_cls=bpg.Prover, ctx=ctx).prover.template(ctx)
    refs = [Ref(G.hand10(i, v, False, prover_cls=bpg.Prover, ctx=ctx), "hand %d" % k, gens) for k, (i, v) in enumerate(zip(G.HAND_INPUTS, G.HAND_VALUES))]
    yield tmpl, refs
    tmpl.free()


def test_hand10_single_proofs(ctx, hand):
    tmpl, refs = hand
    assert tmpl.n_inputs == 4 and tmpl.n_gates >= 10
    for k in (1, 2, 3, 0):
        r, ins = refs[k], [sc(x) for x in G.HAND_INPUTS[k]]
        tmpl.assign(r.inst.v, inputs=ins)
        assert tmpl.check().ok
        proof, after = tmpl.prove(r.state, r.inst.v_blinding, rng(r.tag))
        assert proof == r.proof and after == r.state_after, "vector %d: the template's proof differs from the oracle's proof of the assembly with constants" % k
        assert tmpl.verify(r.state, r.coms, proof) == 0
        tmpl.set_inputs([sc(x) for x in G.HAND_INPUTS[(k + 1) % 4]])               # the verifier's half: other inputs, another statement
        assert tmpl.verify(r.state, r.coms, proof) == 3
        assert ctx.verify_flat(r.inst, r.state, r.coms, proof) == 0


def test_hand10_checkpointed(ctx, hand):
    """the gate over m3's output reads the caller's value"""
    _, refs = hand
    tmpl = G.hand10(G.HAND_INPUTS[0], G.HAND_VALUES[0], True, prover_cls=bpg.Prover, ctx=ctx).prover.template(ctx, checkpoints=[G.HAND_CHECKPOINT])
    try:
        r, ins = refs[3], [sc(x) for x in G.HAND_INPUTS[3]]
        good = r.inst.aO[32 * 3:32 * 4]
        tmpl.assign(r.inst.v, checkpoints=[good], inputs=ins)
        assert tmpl.prove(r.state, r.inst.v_blinding, rng(r.tag)) == (r.proof, r.state_after)
        with pytest.raises(bpg.BpgError) as e:
            tmpl.assign(r.inst.v, checkpoints=[sc(5)], inputs=ins)
        assert e.value.status == MISMATCH and e.value.first_mismatch == 0
    finally:
        tmpl.free()


@pytest.mark.parametrize("K", [3, 65])
def test_hand10_lockstep_batch(ctx, hand, K):
    """every item its own inputs and witness, against assign + prove one at a time (item 64: one past a 64-lane block)"""
    tmpl, refs = hand
    ins = [[sc((7 * k + 1) * 2**(3 * k % 250) % L), sc(k % 2), sc(L - 1 - k), sc(2**252 + 9 + k)] for k in range(K)]
    cases = [G.hand10([int.from_bytes(x, "little") for x in ins[k]], ((k + 2) % L, (L - 5 * k - 1) % L), False, prover_cls=bpg.Prover, ctx=ctx, tag="b%d" % k)
             for k in range(K)]
    rs = [Ref(c, "hand batch %d" % k) for k, c in enumerate(cases)]
    pre = state_before(b"hand10")
    for commit in (False, True):
        items = [(r.inst.v, [], pre if commit else r.state, r.inst.v_blinding, rng(r.tag), 0, None, ins[k]) for k, r in enumerate(rs)]
        res = tmpl.prove_batch_inputs(items, commit=commit)
        for k in (range(K) if K < 10 else (0, 1, 31, 63, 64)):
            tmpl.assign(rs[k].inst.v, inputs=ins[k])
            assert tuple(res[k][:2]) == tuple(tmpl.prove(rs[k].state, rs[k].inst.v_blinding, rng(rs[k].tag))), "item %d (commit=%d)" % (k, commit)
            assert ctx.verify_flat(rs[k].inst, rs[k].state, rs[k].coms, res[k][0]) == 0, "item %d: the assembly with constants rejects the proof" % k
            if commit:
                assert res[k][2] == rs[k].coms
    # the last item against the oracle's proof of its assembly with constants
    k = K - 1
    rc, want, _ = O.prove(O.Gens(16), rs[k].state, to_oracle(rs[k].inst), rs[k].inst.v_blinding, rng(rs[k].tag), O.FLAG_FAST_MSM)
    assert rc == 0 and res[k][0] == want


# ------------------------------------------------------------------------------------------------ 2. depth 2: the four leaves of one resident tree, one wave
class Depth2:
    def __init__(self, ctx):
        self.leaves = G.sample_leaves(4, "gpu-d2")
        self.tree = ctx.merkle_tree(self.leaves)
        self.root = self.tree.root()
        idx = [0, 1, 2, 3]
        self.paths, self.nodes, self.inputs = self.tree.paths(idx), self.tree.path_nodes(idx), self.tree.path_inputs(idx)
        g0 = G.path_gated(ctx, 0, self.leaves[0], self.paths[0], self.root, prover_cls=bpg.Prover)
        self.ck_vars = G.node_checkpoints(g0.prover)
        self.plain = g0.prover.template(ctx)
        self.ckd = g0.prover.template(ctx, checkpoints=self.ck_vars)
        gens = O.Gens(4096)
        self.refs = [Ref(G.path_reference(ctx, i, self.leaves[i], self.paths[i], self.root, prover_cls=bpg.Prover), "d2 leaf %d" % i, gens) for i in idx]

    def items(self, commit, cks):
        pre = state_before(G.PATH_LABEL)
        return [(r.inst.v, [], pre if commit else r.state, r.inst.v_blinding, rng(r.tag), 0, self.nodes[i] if cks else None, self.inputs[i])
                for i, r in enumerate(self.refs)]

    def free(self):
        self.plain.free(); self.ckd.free(); self.tree.free()


@pytest.fixture(scope="module")
def d2(ctx):
    s = Depth2(ctx)
    yield s
    s.free()


def launches(ctx, call, names=("k_input_slots", "k_witness_eval_batch", "k_witness_eval", "k_vw_flatten", "k_vw_tails")):
    ctx.profile_set(2)
    try:
        res = call()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: rep.get(k, {"count": 0})["count"] for k in names}


def test_tree_feeds_the_helper(d2):
    for i in range(4):
        assert d2.inputs[i] == bpg.merkle_path_inputs(i, d2.paths[i], d2.root) and len(d2.inputs[i]) == 9
        assert d2.leaves[i] == bytes(d2.refs[i].inst.v) and d2.nodes[i][-1] == d2.root


@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("cks", [False, True])
def test_depth2_wave(ctx, d2, commit, cks):
    tmpl = d2.ckd if cks else d2.plain
    res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(d2.items(commit, cks), commit=commit))
    assert n["k_input_slots"] == 1 and n["k_witness_eval"] == 0 and n["k_witness_eval_batch"] == (2 if cks else 4), n      # one wave; a launch per level
    for i, r in enumerate(d2.refs):
        assert res[i][0] == r.proof, "leaf %d: the proof differs from the oracle's proof of the reference pattern assembly" % i
        assert res[i][1] == r.state_after
        if commit:
            assert res[i][2] == r.coms


def test_depth2_wrong_checkpoint_fails_its_item_alone(ctx, d2):
    items = d2.items(False, True)
    items[2] = items[2][:6] + ([d2.nodes[2][0], sc(7)],) + items[2][7:]
    res, st, first = d2.ckd.prove_batch_inputs(items, return_status=True)
    assert st == [0, 0, MISMATCH, 0] and first == [None, None, 1, None]
    assert res[2][0] is None and [res[i][0] for i in (0, 1, 3)] == [d2.refs[i].proof for i in (0, 1, 3)]


def test_depth2_check(ctx, d2):
    r = d2.refs[1]
    d2.plain.assign(r.inst.v, inputs=d2.inputs[1])
    assert d2.plain.check().ok
    d2.plain.assign(sc(int.from_bytes(d2.leaves[1], "little") + 1), inputs=d2.inputs[1])           # another leaf: every multiplier holds, the root row does not
    rep = d2.plain.check()
    assert rep.bad_multipliers == 0 and rep.bad_rows == 1 and rep.rows == [d2.plain.q - 1], rep


def test_depth2_verification(ctx, d2):
    import ctypes as C
    import verify_wave_cases as W
    tmpl = d2.plain
    tmpl.set_inputs(d2.inputs[0])
    z = sc(W.filler(b"gates z"))
    before = tmpl.test_weights(z)
    item = lambda i, inputs: (d2.refs[i].state, d2.refs[i].coms, d2.refs[i].proof, bytes([i + 1]) * 32, 0, None, b"".join(inputs))
    (st, states), n = launches(ctx, lambda: tmpl.verify_batch([item(i, d2.inputs[i]) for i in range(4)], batch_seed=bytes(32)))
    assert st == [0, 0, 0, 0] and n["k_vw_flatten"] == 1 and n["k_vw_tails"] == 1 and n["k_input_slots"] == 0, (st, n)
    assert tmpl.test_weights(z) == before, "an accepted call changed the circuit's standing slots"
    # one flipped index bit (item 1 claims leaf 3's place beside the same siblings), one swapped sibling (item 2): each rejected alone
    flipped = bpg.merkle_path_inputs(1 ^ 2, d2.paths[1], d2.root)
    swapped = bpg.merkle_path_inputs(2, d2.paths[2][::-1], d2.root)
    bad = {1: flipped, 2: swapped}
    st, states2 = tmpl.verify_batch([item(i, bad.get(i, d2.inputs[i])) for i in range(4)], batch_seed=bytes(32))
    assert st == [0, 3, 3, 0], st
    assert tmpl.test_weights(z) == before, "a rejected call changed the circuit's standing slots"
    for i in range(4):                                                                                      # what set_inputs + verify gives for the item alone
        for inputs, want in ((d2.inputs[i], 0),) + (((bad[i], 3),) if i in bad else ()):
            tmpl.set_inputs(inputs)
            ts = C.create_string_buffer(bytes(d2.refs[i].state), 203)
            s = bpg.lib().bpg_r1cs_verify_resident(ctx._h, tmpl._h, ts, C.c_uint64(1), d2.refs[i].coms, d2.refs[i].proof, C.c_uint64(len(d2.refs[i].proof)),
                                                   bytes([i + 1]) * 32, C.c_uint32(0))
            assert s == want and (want or ts.raw[:203] == states[i]), (i, s)
    # the wave kernels on chosen challenges: every item's weights are the integer model's over the REFERENCE assembly of its index
    rows = [W.Rows(r.inst) for r in d2.refs]
    recs = W.challenge_set("hashed", 12, 4, b"gates")
    g, h, slots, ev = tmpl.test_verify_wave_scalars([W.record_bytes(r) for r in recs], inputs=[b"".join(x) for x in d2.inputs])
    wg, wh, wslots = W.wave_bytes(rows, recs)
    assert (g, h) == (wg, wh), "accumulators: an item's variable columns did not read its own derived slots"
    assert slots == wslots and ev["n_tail"] > 0
    # and per item the slots' w_V and w_c are test_weights(z_k) after set_inputs of that item
    for k in range(4):
        tmpl.set_inputs(d2.inputs[k])
        wL, wR, wO, wV, wc = tmpl.test_weights(W.record_bytes(recs[k])[1])
        assert slots[k][:1] == wV and slots[k][1] == wc, "item %d" % k


def test_refused_on_the_device_too(ctx, d2):
    for call in (lambda: d2.plain.repeat(2), lambda: d2.plain.repeat_inputs(2), lambda: ctx.join([(d2.plain, 2)]), lambda: ctx.join_inputs([(d2.plain, 2)]),
                 lambda: d2.plain.check_batch_inputs([(d2.refs[0].inst.v, [], d2.inputs[0])] * 2)):
        with pytest.raises(bpg.BpgError) as e:
            call()
        assert e.value.status == 4 and "gated variables" in str(e.value)


# ------------------------------------------------------------------------------------------------ 3. depth 3: a grown tree (child process, census)
def case_grown_tree():
    ok = {}
    ctx = bpg.Context(0)
    cap = 8192
    ctx.gens_ensure(cap)
    leaves = G.sample_leaves(6, "gpu-d3")
    tree = ctx.merkle_tree(leaves[:5], depth=3, empty=sc(13))
    idx = [0, 2, 5, 7]
    value = lambda i: tree.nodes(3, i, 1)[0]                     # leaves 5 and 7 hold the empty value until something is appended there
    g0 = G.path_gated(ctx, 0, value(0), tree.paths([0])[0], tree.root(), prover_cls=bpg.Prover)
    tmpl = g0.prover.template(ctx, checkpoints=G.node_checkpoints(g0.prover))
    pre = state_before(G.PATH_LABEL)

    def wave(tag):
        root, paths, nodes, inputs = tree.root(), tree.paths(idx), tree.path_nodes(idx), tree.path_inputs(idx)
        blinds = [G.blind(tag, k) for k in range(4)]
        items = [(value(i), [], pre, blinds[k], rng("%s %d" % (tag, k)), 0, nodes[k], inputs[k]) for k, i in enumerate(idx)]
        ctx.profile_set(2)
        res = tmpl.prove_batch_inputs(items, commit=True)
        rep = ctx.profile_report()
        ctx.profile_set(0)
        one_wave = rep["k_witness_eval_batch"]["count"] == 2 and rep.get("k_witness_eval", {"count": 0})["count"] == 0
        return root, paths, res, one_wave

    root, paths, res, one_wave = wave("five")
    ok["one wave of four leaves"] = one_wave and all(r[0] is not None for r in res)
    ok["the reference circuits accept"] = all(reference_verdict(ctx, i, res[k][2], paths[k], root, res[k][0], cap) for k, i in enumerate(idx))
    ok["another index rejects"] = not reference_verdict(ctx, 3, res[1][2], paths[1], root, res[1][0], cap)
    first, new_root = tree.append([leaves[5]], return_root=True)
    ok["append"] = first == 5 and new_root == tree.root() != root
    ok["old proofs fail under the new root"] = not any(reference_verdict(ctx, i, res[k][2], paths[k], new_root, res[k][0], cap) for k, i in enumerate(idx))
    root2, paths2, res2, one_wave2 = wave("six")
    ok["a wave against the new root"] = one_wave2 and root2 == new_root and value(5) == leaves[5] and \
        all(reference_verdict(ctx, i, res2[k][2], paths2[k], root2, res2[k][0], cap) for k, i in enumerate(idx))
    st, _ = tmpl.verify_batch([(_after_commit(pre, res2[k][2]), res2[k][2], res2[k][0], None, 0, None, b"".join(x)) for k, x in enumerate(tree.path_inputs(idx))])
    ok["verify_batch under the tree's inputs"] = st == [0, 0, 0, 0]
    tmpl.free(); tree.free(); ctx.close()
    return {"ok": ok, "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}


def _after_commit(pre, com):
    """the transcript after the one commitment of a path statement"""
    t = bpg.Transcript(G.PATH_LABEL)
    v = bpg.Verifier(t)
    v.commit(com)
    return t.state


def test_grown_tree_in_a_process_of_its_own():
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_gates_gpu.py"), "child"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(out["ok"].values()), out
    assert out["end"] == [0] * 6, out


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    print(json.dumps(case_grown_tree()))
