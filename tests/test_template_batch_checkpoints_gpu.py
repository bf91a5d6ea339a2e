"""Checkpointed templates in lockstep batches on the GPU (bpg_r1cs_prove_template_batch_checkpointed, k_witness_ck_verify_batch): K hash-chain proofs per
wave, their witnesses evaluated in the one or two levels of the checkpointed schedule.

The yardstick is always the EXISTING path, never the new call: the host assembly of the same witness, uploaded and proved with the same transcript state,
blindings and rng seed (host_proof).  A checkpointed assign + prove of the item alone must equal it too.  The checkpoint values never come from the
circuit: Python integers for the chain, the native host sponge for the preimage (checkpoint_cases.py), the resident tree for the paths.

Shapes are the smallest that take every branch: the 36-multiplier chain (5 checkpoints, one level) with K = 3 and K = 70 (two blocks of item lanes, the
second one partial), depth-3 paths (N = 8192, two levels), a 3-block preimage (one level).  The wave cut and the fallback are read at context creation:
those tests make a context of their own under the environment they need."""
import ctypes as C
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
import checkpoint_cases as CK

pytestmark = pytest.mark.gpu
SEED = hashlib.sha256(b"template batch checkpoints").digest()
MISMATCH, MISSING, INVALID = 9, 5, 4
NONE = 2**64 - 1
KERNELS = ("k_witness_eval_batch", "k_witness_ck_verify_batch", "k_witness_eval", "k_witness_ck_verify", "k_bt_commit_v", "k_pedersen")


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(8192)
    yield c
    c.close()


def state_before(label):
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(label)
    bpg.Prover(None, t)
    return t.state


def host_proof(ctx, a, flags=0):
    """the existing path: the host-assembled instance, uploaded and proved -> (proof, transcript state after)"""
    inst = a.prover.instance()
    res = ctx.upload(inst)
    out = res.prove(a.transcript.state, inst.v_blinding, SEED, flags=flags)
    res.free()
    return out


def launches(ctx, fn):
    """fn() under the all-kernels profile -> (its result, launches of the kernels this file counts)"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: rep.get(k, {"count": 0})["count"] for k in KERNELS}


class Item:
    """one witness: the host assembly `a` (its commitments and post-commit transcript come from the existing Prover.commit path) and what the host proves"""
    def __init__(self, ctx, a, label, param=None):
        self.a, self.inst = a, a.prover.instance()
        self.param = CK.constant_term(self.inst, CK.last_row(a)) if param is None else param
        self.pre, self.post = state_before(label), a.transcript.state
        self.coms = b"".join(a.commitments)
        out = C.create_string_buffer(203)                                                   # the label is the circuit's: pre + the "V" appends = post
        assert bpg.lib().bpg_test_append_commitments(self.pre, C.c_uint64(self.inst.m), self.coms, out) == 0 and out.raw == self.post
        self.ck = list(a.ck_values)
        self.want = host_proof(ctx, a)

    def item(self, commit, ck=None, flags=0):
        return (self.inst.v, [self.param], self.pre if commit else self.post, self.inst.v_blinding, SEED, flags, self.ck if ck is None else ck)

    def result(self, commit, want=None):
        want = self.want if want is None else want
        return want + (self.coms,) if commit else want


@pytest.fixture(scope="module")
def chains(ctx):
    """70 witnesses of the chain (seeds 2..71) with their host proofs, computed once; the template is made from seed 1"""
    return [Item(ctx, CK.chain(ctx, seed=2 + k), b"CheckpointChain") for k in range(70)]


def chain_templates(ctx):
    base = CK.chain(ctx, seed=1)
    rows = [CK.last_row(base)]
    return base.prover.template(ctx, param_rows=rows, checkpoints=base.ck_vars), base.prover.template(ctx, param_rows=rows)


@pytest.fixture(scope="module")
def chain_ck(ctx):
    ck, plain = chain_templates(ctx)
    yield ck, plain
    ck.free(); plain.free()


@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("K", [3, 70])
def test_chain(ctx, chains, chain_ck, K, commit):
    ck, _ = chain_ck
    assert ck.n == 36 and ck.n_ck == 5 and len({c.inst.v for c in chains}) == 70
    got, n = launches(ctx, lambda: ck.prove_batch_checkpointed([c.item(commit) for c in chains[:K]], commit=commit))
    assert n["k_witness_eval_batch"] == 1 and n["k_witness_ck_verify_batch"] == 1, n          # one wave, one level, one comparison
    assert n["k_witness_eval"] == 0 and n["k_witness_ck_verify"] == 0 and n["k_bt_commit_v"] == (1 if commit else 0), n
    assert len(got) == K
    for k in range(K):
        assert got[k] == chains[k].result(commit), "item %d of %d: proof, out-state or commitments differ from the host prover's" % (k, K)
    # the item alone: checkpointed assign + prove
    c = chains[K - 1]
    ck.assign(c.inst.v, [c.param], checkpoints=c.ck)
    assert ck.prove(c.post, c.inst.v_blinding, SEED) == c.want


def test_paths_from_resident_trees(ctx):
    depth, index, K = 3, 5, 5
    base = CK.path(ctx, index, depth=depth, seed=1)
    rows = [CK.last_row(base)]
    ck, plain = base.prover.template(ctx, param_rows=rows, checkpoints=base.ck_vars), base.prover.template(ctx, param_rows=rows)
    trees = []
    try:
        items = []
        for s in range(2, 2 + K):
            leaves = [bpg.be_to_scalar(b) for b in CK.tree_leaves(s, 1 << depth)]
            tree = ctx.merkle_tree(leaves); trees.append(tree)
            sib = tree.paths([index])[0]
            values = [leaves[index] if what == "leaf" else sib[k] for what, k in base.order]
            a = CK.path_from(ctx, CK.host_tree(leaves), index, "ck-batch-%d" % s)          # the host's commitments and transcript for the same values
            assert a.values == values and a.root == tree.root()
            it = Item(ctx, a, b"MerklePath", param=bpg.scalar_op("sub", bytes(32), tree.root()))
            assert it.param == CK.constant_term(it.inst, CK.last_row(a))
            it.ck = tree.path_nodes([index])[0]
            assert it.ck == a.ck_values
            items.append(it)
        assert ck.n == 5832 and ck.n_ck == 3 and len({it.inst.v for it in items}) == K
        for commit in (False, True):
            got, n = launches(ctx, lambda: ck.prove_batch_checkpointed([it.item(commit) for it in items], commit=commit))
            assert n["k_witness_eval_batch"] == 2 and n["k_witness_ck_verify_batch"] == 1 and n["k_witness_eval"] == 0, n      # one wave, two levels
            assert got == [it.result(commit) for it in items]
        want, n = launches(ctx, lambda: plain.prove_batch([it.item(False)[:6] for it in items]))
        # the same circuit without checkpoints: the levels of ITS schedule, depth + 1 = 4 (a node's first block is level with the block that made its child's
        # digest ready - tests/test_template_checkpoints_host.py test_merkle_path_two_levels - not the 2 x depth a level per block would give)
        assert n["k_witness_eval_batch"] == depth + 1 > 2 and n["k_witness_ck_verify_batch"] == 0, n
        assert want == [it.want for it in items]
        for it in items:
            proof = it.want[0]
            ck.assign(it.inst.v, [it.param], checkpoints=it.ck)                                 # the item alone; and the parameter slots verify() reads
            assert ck.prove(it.post, it.inst.v_blinding, SEED) == it.want
            assert ck.verify(it.post, it.coms, proof) == 0
            assert ctx.verify_flat(it.inst, it.post, it.coms, proof) == 0
    finally:
        for c in [ck, plain] + trees:
            c.free()


def test_preimage(ctx):
    base = CK.preimage3(ctx, seed=1)
    rows = [CK.last_row(base)]
    ck = base.prover.template(ctx, param_rows=rows, checkpoints=base.ck_vars)
    try:
        items = [Item(ctx, CK.preimage3(ctx, seed=s), b"MiMCHash") for s in (2, 3)]
        assert items[0].post != items[0].pre and ck.n_ck == 3
        for commit in (False, True):
            got, n = launches(ctx, lambda: ck.prove_batch_checkpointed([it.item(commit) for it in items], commit=commit))
            assert n["k_witness_eval_batch"] == 1 and n["k_witness_ck_verify_batch"] == 1 and n["k_witness_eval"] == 0, n
            assert got == [it.result(commit) for it in items]
    finally:
        ck.free()


def wrong(b):
    return bpg.scalar_op("add", b, bpg.scalar_from_int(1))


def mismatch_items(chains, commit, K=70, bad=((66, 2), (69, 4))):
    items = [c.item(commit) for c in chains[:K]]
    for k, j in bad:
        vals = list(chains[k].ck); vals[j] = wrong(vals[j])
        if j < 4:
            vals[4] = wrong(vals[4])                                                        # a later one as well: the lowest is reported
        items[k] = chains[k].item(commit, ck=vals)
    return items


@pytest.mark.parametrize("commit", [False, True])
def test_mismatch_fails_alone(ctx, chains, chain_ck, commit):
    ck, _ = chain_ck
    K, m = 70, 6
    items = mismatch_items(chains, commit)
    arr, keep = ck._template_items([it[:6] for it in items], bpg._TemplateCkItem)
    coms = [C.create_string_buffer(b"\xa5" * (32 * m), 32 * m) for _ in range(K)]
    firsts = [C.c_uint64(7) for _ in range(K)]
    cks = [b"".join(it[6]) for it in items]
    for k in range(K):
        C.memset(keep[k][1], 0xa5, len(keep[k][1]))
        arr[k].commitments_out = C.cast(coms[k], C.c_void_p); arr[k].ck_values = cks[k]; arr[k].first_mismatch = C.pointer(firsts[k])
    arr[3].proof_len = None                                                                 # item 3 fails on its own: a NULL proof length
    status = (C.c_int32 * K)(*[77] * K)
    c0 = chains[0]
    ck.assign(c0.inst.v, [c0.param], checkpoints=c0.ck)                                     # a witness is resident before the batch ...
    rc = bpg.lib().bpg_r1cs_prove_template_batch_checkpointed(ctx._h, ck._h, C.c_uint64(K), arr, C.c_int32(1 if commit else 0), status)
    assert rc == INVALID and b"item 3" in bpg.lib().bpg_last_error()                        # the first failing item's status is the call's
    assert [(k, s) for k, s in enumerate(status) if s != 0] == [(3, INVALID), (66, MISMATCH), (69, MISMATCH)]
    assert [(k, f.value) for k, f in enumerate(firsts) if f.value != NONE] == [(66, 2), (69, 4)]
    for k in range(K):
        ts, out, ln = keep[k][:3]
        if k in (3, 66, 69):
            assert ts.raw[:203] == items[k][2], "item %d: a failed item's transcript is left as given" % k
            assert out.raw == b"\xa5" * len(out) and ln.value == len(out), "item %d: nothing is written to a failed item's proof buffer" % k
            assert coms[k].raw == b"\xa5" * (32 * m), "item %d: no commitment is written for a failed item" % k
        else:
            assert (out.raw[:ln.value], ts.raw[:203]) == chains[k].want, "item %d: proof or out-state differ from the host prover's" % k
            assert coms[k].raw == (chains[k].coms if commit else b"\xa5" * (32 * m)), "item %d: commitments" % k
    with pytest.raises(bpg.BpgError) as e:                                                  # ... and none after it
        ck.prove(c0.post, c0.inst.v_blinding, SEED)
    assert e.value.status == MISSING


def test_binding_conventions(ctx, chains, chain_ck):
    ck, _ = chain_ck
    items = mismatch_items(chains, True)
    with pytest.raises(bpg.BpgError) as e:
        ck.prove_batch_checkpointed(items, commit=True)
    assert e.value.status == MISMATCH and e.value.item == 66 and e.value.first_mismatch == 2, str(e.value)
    assert "item 66" in str(e.value) and "checkpoint 2" in str(e.value), str(e.value)
    items[5] = items[5][:6] + (None,)                                                       # no checkpoint values: that item alone, INVALID_ARGUMENT
    res, st, first = ck.prove_batch_checkpointed(items, commit=True, return_status=True)
    assert [(k, s) for k, s in enumerate(st) if s] == [(5, INVALID), (66, MISMATCH), (69, MISMATCH)]
    assert [(k, f) for k, f in enumerate(first) if f is not None] == [(66, 2), (69, 4)]
    for k in range(70):
        assert res[k] == ((None, chains[k].pre, None) if st[k] else chains[k].result(True)), k
    # x + l (below 2^255) in place of x is the same scalar: no mismatch, the same bytes
    c = chains[7]
    vals = [(int.from_bytes(b, "little") + bpg.L).to_bytes(32, "little") if int.from_bytes(b, "little") + bpg.L < 1 << 255 else b for b in c.ck]
    assert vals != c.ck
    assert ck.prove_batch_checkpointed([c.item(False, ck=vals)]) == [c.want]
    assert ck.prove_batch_checkpointed([]) == []
    # the frozen calls still refuse the checkpointed template
    with pytest.raises(bpg.BpgError) as e:
        ck.prove_batch([c.item(False)[:6]])
    assert e.value.status == INVALID


def test_a_template_without_checkpoints_is_the_existing_call(ctx, chains, chain_ck):
    _, plain = chain_ck
    cs = chains[:3]
    want = plain.prove_batch([c.item(False)[:6] for c in cs])
    want_commit = plain.prove_batch_commit([c.item(True)[:6] for c in cs])
    assert want == [c.want for c in cs] and want_commit == [c.result(True) for c in cs]
    for ckv in (None, []):
        got, n = launches(ctx, lambda: plain.prove_batch_checkpointed([c.item(False)[:6] + (ckv,) for c in cs]))
        assert got == want and n["k_witness_ck_verify_batch"] == 0 and n["k_witness_eval_batch"] == 6, n       # the schedule without checkpoints: six levels
    res, st, first = plain.prove_batch_checkpointed([c.item(True)[:6] + (None,) for c in cs], commit=True, return_status=True)
    assert res == want_commit and st == [0, 0, 0] and first == [None] * 3


@pytest.mark.parametrize("setting", ["one-item-per-wave", "fallback", "expanded-among-lockstep"])
def test_waves_and_fallback(chains, monkeypatch, setting):
    """BPG_BATCH_WAVE_MB=0: one proof per wave - a launch of each witness kernel per item, and a mismatch in the last wave fails alone.  BPG_TT_ORIG_LG=0: no
    lockstep path - every item is assign_checkpointed + prove, same bytes, same reporting.  One BPG_FLAG_EXPANDED_BLINDING item among lockstep items is
    proved on that path alone."""
    K = 6
    for name, value in {"one-item-per-wave": {"BPG_BATCH_WAVE_MB": "0"}, "fallback": {"BPG_TT_ORIG_LG": "0"}, "expanded-among-lockstep": {}}[setting].items():
        monkeypatch.setenv(name, value)
    own = bpg.Context(0)
    ck = None
    try:
        own.gens_ensure(64)
        ck, plain = chain_templates(own)
        plain.free()
        flags = [4 if (setting == "expanded-among-lockstep" and k == 2) else 0 for k in range(K)]
        want = {2: host_proof(own, chains[2].a, flags=4)} if setting == "expanded-among-lockstep" else {}
        for commit in (False, True):
            items = [c.item(commit, flags=f) for c, f in zip(chains[:K], flags)]
            vals = list(chains[K - 1].ck); vals[3] = wrong(vals[3])
            items[K - 1] = chains[K - 1].item(commit, ck=vals)
            (res, st, first), n = launches(own, lambda: ck.prove_batch_checkpointed(items, commit=commit, return_status=True))
            print(setting, commit, n)
            lock, single = {"one-item-per-wave": (K, 0), "fallback": (0, K), "expanded-among-lockstep": (1, 1)}[setting]
            assert n["k_witness_eval_batch"] == lock and n["k_witness_ck_verify_batch"] == lock, n
            assert n["k_witness_eval"] == single and n["k_witness_ck_verify"] == single, n
            assert st == [0] * (K - 1) + [MISMATCH] and first == [None] * (K - 1) + [3]
            with pytest.raises(bpg.BpgError) as e:                                          # the same call raising: the message names item and checkpoint
                ck.prove_batch_checkpointed(items, commit=commit)
            assert e.value.status == MISMATCH and (e.value.item, e.value.first_mismatch) == (K - 1, 3), str(e.value)
            assert "item %d" % (K - 1) in str(e.value) and "checkpoint 3" in str(e.value), str(e.value)
            for k in range(K - 1):
                assert res[k] == chains[k].result(commit, want.get(k)), "%s, item %d" % (setting, k)
            assert res[K - 1] == ((None, chains[K - 1].pre, None) if commit else (None, chains[K - 1].post))
    finally:
        if ck is not None:
            ck.free()
        own.close()


def test_resources_return(ctx, chains):
    def cycle():
        ck, plain = chain_templates(ctx)
        for commit in (False, True):
            res, st, _ = ck.prove_batch_checkpointed(mismatch_items(chains, commit, K=5, bad=((4, 1),)), commit=commit, return_status=True)
            assert st == [0, 0, 0, 0, MISMATCH]
        ck.free(); plain.free()
    cycle()                                                                                 # the context's own staging buffers grow once
    start = bpg.live_resources()
    cycle()
    assert bpg.live_resources() == start
