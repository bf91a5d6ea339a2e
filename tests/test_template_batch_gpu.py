"""Lockstep template batches on the GPU (bpg_r1cs_prove_template_batch): K fresh witnesses of one circuit template, evaluated on the device in shared
launches and proved in lockstep, give exactly the proofs and transcript states of the EXISTING path - host assembly of each witness, bpg_r1cs_upload,
bpg_r1cs_prove_resident (`host_proof` of tests/test_template_gpu.py) - and the CPU oracle's verifier accepts them.  The new path is never compared
with itself; where the contract is "assign + prove_resident one by one" (the fallback), that pair is the yardstick, itself pinned to host_proof by
tests/test_template_gpu.py.

All on the 8-leaf Merkle template (n = 13,608, N = 2^14, 14 segments on 6 levels) with the root's row as the parameter, unless said otherwise."""
import ctypes as C
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
from test_template_gpu import constant_term, last_row, to_oracle

pytestmark = pytest.mark.gpu
L = bpg.L
SEEDS = list(range(2, 14))
LEVELS = 6
N = 1 << 14


def rng(seed):
    return hashlib.sha256(("template batch %s" % seed).encode()).digest()


class Case:
    """one witness of the 8-leaf tree: host assembly, and the existing path's proof per dialect (made on demand, cached)"""
    def __init__(self, ctx, seed, leaves=8):
        self.ctx, self.seed = ctx, seed
        self.a = workloads.merkle_full_tree(ctx, leaves=leaves, seed=seed)
        self.inst = self.a.prover.instance()
        self.state = self.a.transcript.state
        self.param = constant_term(self.inst, last_row(self.a))
        self._want = {}

    def item(self, flags=0):
        return (self.inst.v, [self.param], self.state, self.inst.v_blinding, rng(self.seed), flags)

    def host_proof(self, flags=0):
        """the existing path: the host-assembled instance, uploaded and proved -> (proof, transcript state after)"""
        if flags not in self._want:
            res = self.ctx.upload(self.inst)
            self._want[flags] = res.prove(self.state, self.inst.v_blinding, rng(self.seed), flags)
            res.free()
        return self._want[flags]


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    return {s: Case(ctx, s) for s in SEEDS}


@pytest.fixture(scope="module")
def tmpl(ctx, cases):
    """made WITHOUT a witness from seed 2's shape"""
    c = cases[2]
    t = make_template(ctx, c)
    yield t
    t.free()


def make_template(ctx, c):
    prog = c.a.prover.witness_program(); prog.param_rows = [last_row(c.a)]
    cs, cp, h = c.inst.cstruct(), prog.cstruct(), C.c_void_p()
    cs.aL = cs.aR = cs.aO = None
    assert bpg.lib().bpg_r1cs_upload_template(ctx._h, C.byref(cs), C.byref(cp), C.byref(h)) == 0, bpg.lib().bpg_last_error()
    return bpg.ResidentCircuit(ctx, h, c.inst.n, c.inst.m, n_params=1)


def witness_launches(ctx, tmpl, items):
    """(results, launches of k_witness_eval_batch, launches of k_witness_eval) of one batch"""
    ctx.profile_set(2)
    res = tmpl.prove_batch(items)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    return res, rep.get("k_witness_eval_batch", {"count": 0})["count"], rep.get("k_witness_eval", {"count": 0})["count"]


def test_bytes_of_twelve_items(ctx, cases, tmpl):
    assert cases[2].inst.n == 13608
    got = tmpl.prove_batch([cases[s].item() for s in SEEDS])
    ogens = O.Gens(N)
    for s, (proof, state) in zip(SEEDS, got):
        want = cases[s].host_proof()
        assert proof == want[0], "seed %d: the template batch and the host assembly give different proofs" % s
        assert state == want[1], "seed %d: transcript state after" % s
        c = cases[s]
        assert O.verify(ogens, c.state, to_oracle(c.inst), b"".join(c.a.commitments), proof) == 0, "seed %d: the oracle rejects the proof" % s


def test_composition_does_not_matter(ctx, cases, tmpl):
    want = cases[5].host_proof()
    for batch in ([5], [4, 5, 6], SEEDS):
        got = tmpl.prove_batch([cases[s].item() for s in batch])
        assert got[batch.index(5)] == want, "item 5 in a batch of %d" % len(batch)


def test_launches_are_shared(ctx, cases, tmpl):
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [cases[s].item() for s in SEEDS])
    assert nbatch == LEVELS and nsingle == 0, (nbatch, nsingle)
    assert res == [cases[s].host_proof() for s in SEEDS]
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [cases[3].item()])
    assert nbatch == LEVELS and nsingle == 0 and res == [cases[3].host_proof()]


@pytest.mark.parametrize("setting", ["one-per-wave", "several-waves"])
def test_waves_keep_the_bytes(monkeypatch, cases, setting):
    """BPG_BATCH_WAVE_MB=0: one proof per wave (12 waves).  The engine estimates about 30 N x 32 B of device state per item (15.7 MB at N = 2^14; its
    exact figure adds the rows and coefficients of the instance, a few MB): a cap of 4.5 such estimates holds at least two and at most four items, so the
    twelve items run in 3 to 6 waves of more than one item each.  The cut is read off the launch count: 6 level launches per wave."""
    mb = 0 if setting == "one-per-wave" else (45 * 30 * N * 32 // 10) >> 20
    monkeypatch.setenv("BPG_BATCH_WAVE_MB", str(mb))
    ctx = bpg.Context(0)
    ctx.gens_ensure(N)
    t = make_template(ctx, cases[2])
    res, nbatch, nsingle = witness_launches(ctx, t, [cases[s].item() for s in SEEDS])
    print("BPG_BATCH_WAVE_MB=%d: %d launches of k_witness_eval_batch" % (mb, nbatch))
    assert nsingle == 0 and nbatch % LEVELS == 0
    waves = nbatch // LEVELS
    assert waves == 12 if setting == "one-per-wave" else 2 <= waves <= 6, waves
    assert res == [cases[s].host_proof() for s in SEEDS]
    t.free(); ctx.close()


def test_dialects_mixed_in_one_batch(ctx, cases, tmpl):
    seeds = SEEDS[:8]
    got = tmpl.prove_batch([cases[s].item(flags=k % 4) for k, s in enumerate(seeds)])
    for k, s in enumerate(seeds):
        assert got[k] == cases[s].host_proof(flags=k % 4), "seed %d under flags %d" % (s, k % 4)


def assign_and_prove(t, c, flags=0):
    t.assign(c.inst.v, [c.param])
    return t.prove(c.state, c.inst.v_blinding, rng(c.seed), flags)


def test_fallback_expanded_blinding_inside_a_lockstep_batch(ctx, cases, tmpl):
    """one item with BPG_FLAG_EXPANDED_BLINDING (4) takes assign + prove_resident inside the call; the others stay in lockstep"""
    seeds = SEEDS[:5]
    want4 = assign_and_prove(tmpl, cases[4], flags=4)
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [cases[s].item(flags=4 if s == 4 else 0) for s in seeds])
    assert nbatch == LEVELS and nsingle == LEVELS
    for s, r in zip(seeds, res):
        assert r == (want4 if s == 4 else cases[s].host_proof()), "seed %d" % s
    with pytest.raises(bpg.BpgError) as e:                                   # no witness left behind by the fallback either
        tmpl.prove(cases[4].state, cases[4].inst.v_blinding, rng(4))
    assert e.value.status == 5


def test_fallback_large_template():
    """64 leaves: N = 2^17, above the lockstep path - every item is assign + prove_resident, one by one (a context of its own: 2^17 generators)"""
    ctx = bpg.Context(0)
    big = [Case(ctx, s, leaves=64) for s in (2, 3, 4)]
    ctx.gens_ensure(big[0].a.gens_capacity)
    t = big[0].a.prover.template(ctx, param_rows=[last_row(big[0].a)])
    want = [assign_and_prove(t, c) for c in big]
    res, nbatch, nsingle = witness_launches(ctx, t, [c.item() for c in big])
    assert res == want
    assert nbatch == 0 and nsingle > 0
    with pytest.raises(bpg.BpgError) as e:
        t.prove(big[0].state, big[0].inst.v_blinding, rng(2))
    assert e.value.status == 5
    t.free(); ctx.close()


def test_an_item_fails_alone(ctx, cases, tmpl):
    seeds = SEEDS[:6]
    items = [cases[s].item() for s in seeds]
    items[3] = (None,) + items[3][1:]                                        # NULL v
    arr, keep = tmpl._template_items(items)
    keep[1][2].value -= 1                                                    # a proof buffer one byte short
    status = (C.c_int32 * 6)(*[77] * 6)
    rc = bpg.lib().bpg_r1cs_prove_template_batch(ctx._h, tmpl._h, C.c_uint64(6), arr, status)
    assert rc == 4 and list(status) == [0, 4, 0, 4, 0, 0], list(status)
    assert b"item 1" in bpg.lib().bpg_last_error()
    for k, s in enumerate(seeds):
        ts, out, ln = keep[k][:3]
        if k in (1, 3):
            assert ts.raw[:203] == cases[s].state                            # a failed item's transcript is left as given
        else:
            assert (out.raw[:ln.value], ts.raw[:203]) == cases[s].host_proof(), "seed %d" % s
    res, st = tmpl.prove_batch(items, return_status=True)                    # the binding's conventions: (None, state as given) for the failed item
    assert st == [0, 0, 0, 4, 0, 0] and res[3] == (None, cases[seeds[3]].state) and res[0] == cases[seeds[0]].host_proof()


def test_template_state_afterwards(ctx, cases, tmpl):
    c = cases[2]
    assert assign_and_prove(tmpl, c) == c.host_proof()                      # a witness is resident ...
    tmpl.prove_batch([cases[3].item(), cases[4].item()])
    with pytest.raises(bpg.BpgError) as e:                                   # ... and gone after a batch
        tmpl.prove(c.state, c.inst.v_blinding, rng(2))
    assert e.value.status == 5
    assert assign_and_prove(tmpl, c) == c.host_proof()
    assert tmpl.prove_batch([]) == []                                        # count == 0 is BPG_OK and touches nothing
    assert tmpl.prove(c.state, c.inst.v_blinding, rng(2)) == c.host_proof()
    plain = ctx.upload(c.inst)
    with pytest.raises(bpg.BpgError) as e:                                   # not a template: the whole call is refused
        plain.prove_batch([c.item()])
    assert e.value.status == 4
    plain.free()


def test_merge_sets_are_dropped(monkeypatch, cases):
    """BPG_MERGE=1 groups equal scalars once per resident witness, at its first proof.  Sets built for one witness must not survive a batch: an equal-leaves
    witness (large sets) is proved, then a batch runs, then a distinct witness is assigned and proved - still the host assembly's bytes.  BPG_TT_ORIG_LG=13
    puts the 2^14 proofs on the bucket-method path, the one that merges; the batch then takes the fallback, which must leave the same state."""
    for env in ({"BPG_MERGE": "1"}, {"BPG_MERGE": "1", "BPG_TT_ORIG_LG": "13"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = bpg.Context(0)
        ctx.gens_ensure(N)
        eq = Case(ctx, None)
        mine = {s: Case(ctx, s) for s in (2, 3)}
        t = make_template(ctx, mine[2])
        assert assign_and_prove(t, eq) == eq.host_proof()
        res = t.prove_batch([mine[2].item(), mine[3].item()])
        assert res == [mine[2].host_proof(), mine[3].host_proof()]
        with pytest.raises(bpg.BpgError) as e:
            t.prove(eq.state, eq.inst.v_blinding, rng(0))
        assert e.value.status == 5
        assert assign_and_prove(t, mine[2]) == mine[2].host_proof()
        assert t.prove(mine[2].state, mine[2].inst.v_blinding, rng(2)) == mine[2].host_proof()
        t.free(); ctx.close()


def test_unreduced_committed_value_in_one_item(ctx):
    """committed values with the top bits set (Scalar::from_bits admits anything below 2^255) in ONE item of a batch: the host assembly's witness"""
    def tree(leaf_ints, tag):
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        leaves = [x.to_bytes(32, "little") for x in leaf_ints]
        coms, vs = p.commit_many(leaves, [workloads.blinding(tag, i) for i in range(len(leaves))])
        probe = bpg.Prover(None, bpg.Transcript(b"probe"))
        bpg.MerkleTree256(bytes(32), leaves, [], "((I I) (I I))").prove(probe, [], [])
        bpg.MerkleTree256(probe.instance().aO[-32:], [], bpg.vars_to_lc(vs), "((W W) (W W))").prove(p, [], [])
        return workloads.Assembled(p, t, coms, 8192, None), b"".join(leaves)
    trees = [tree([11, 12, 13, 14], "u0"), tree([(1 << 254) | (L + 5), (1 << 255) - 19, L, 3 * L + 7], "u1"), tree([21, 22, 23, 24], "u2")]
    assert all(int.from_bytes(trees[1][1][i:i + 32], "little") >= L for i in range(0, 128, 32))
    t = trees[0][0].prover.template(ctx, param_rows=[last_row(trees[0][0])])
    items, want = [], []
    for k, (a, raw) in enumerate(trees):
        inst = a.prover.instance()
        res = ctx.upload(inst); want.append(res.prove(a.transcript.state, inst.v_blinding, rng(100 + k))); res.free()
        items.append((raw, [constant_term(inst, last_row(a))], a.transcript.state, inst.v_blinding, rng(100 + k), 0))      # the unreduced bytes, as handed to commit()
    assert t.prove_batch(items) == want
    a, inst = trees[1][0], trees[1][0].prover.instance()
    assert O.verify(O.Gens(8192), a.transcript.state, to_oracle(inst), b"".join(a.commitments), want[1][0]) == 0
    t.free()
