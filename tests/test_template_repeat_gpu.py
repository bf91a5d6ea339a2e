"""A template repeated K times on the GPU (bpg_r1cs_template_repeat): ONE proof for K witnesses of one circuit shape.

The yardstick is the CPU oracle on the EXISTING host assembly - one prover that commits item by item and assembles the same gadget code K times
(`assemble` of tests/test_template_repeat_host.py): the repeat, built on the device from a template of ONE item and assigned the K items' values, must
give the oracle's proof bytes for that assembly, and the oracle's verifier, the GPU verifier on the host assembly and the GPU verifier on the repeated
handle judge the proofs.  The repeat is never compared with itself.

Sizes: the Merkle pattern ((W W) W) three times (n' = 11,664, N' = 2^14: three schedule levels, a parameter per item); the 8-bit BoundsCheck 65 times
(n' = 1,040, N' = 2,048: one item more than a block of the lane map holds, hints in every item); SetMembership over three elements (n = 6, no power of two)
wherever a small circuit will do."""
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
from test_template_gpu import to_oracle
from test_template_repeat_host import assemble, bounds8_item, constant_term, sc

pytestmark = pytest.mark.gpu
SEED = hashlib.sha256(b"template repeat").digest()


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(16384)
    yield c
    c.close()


class Host:
    """a host assembly of K items in one prover: its instance, the parameter values in item order, the commitments, the transcript after them"""
    def __init__(self, ctx, p, t, rows):
        self.ctx, self.prover = ctx, p
        self.inst = p.instance()
        self.params = [constant_term(self.inst, r) for r in rows]
        self.state = t.state
        self.coms = b"".join(p.commitment(i) for i in range(self.inst.m))
        self.N = 1
        while self.N < self.inst.n:
            self.N *= 2

    def oracle_proof(self):
        rc, proof, state = O.prove(O.Gens(self.N), self.state, to_oracle(self.inst), self.inst.v_blinding, SEED, O.FLAG_FAST_MSM)
        assert rc == 0
        return proof, state

    def upload_proof(self):
        """the existing GPU path on the host assembly (where the oracle's prover is not asked again)"""
        res = self.ctx.upload(self.inst)
        out = res.prove(self.state, self.inst.v_blinding, SEED)
        res.free()
        return out

    def oracle_verify(self, proof):
        return O.verify(O.Gens(self.N), self.state, to_oracle(self.inst), self.coms, proof)

    def assign_and_prove(self, rep):
        rep.assign(self.inst.v, self.params)
        return rep.prove(self.state, self.inst.v_blinding, SEED)


def host(ctx, name, tag, K):
    return Host(ctx, *assemble(name, tag, K, prover_cls=bpg.Prover, ctx=ctx))


def template(ctx, name):
    p, _, rows = assemble(name, "tmpl", 1, prover_cls=bpg.Prover, ctx=ctx)
    return p.template(ctx, param_rows=rows)


def launches(ctx, fn):
    """fn() under the all-kernels profile -> (its result, {kernel: launches})"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: v["count"] for k, v in rep.items()}


@pytest.mark.parametrize("name", ["set3", "bounds8", "merkle3"])
def test_repeat_of_one_is_the_template(ctx, name):
    """repeat(1): assign + prove gives the bytes of the source template's own assign + prove (and those are the host assembly's)"""
    tmpl = template(ctx, name)
    rep = tmpl.repeat(1)
    assert (rep.n, rep.m, rep.n_params) == (tmpl.n, tmpl.m, tmpl.n_params)
    with pytest.raises(bpg.BpgError) as e:                                   # it starts without a witness, though the source holds one
        rep.prove(bytes(203), bytes(32 * rep.m), SEED)
    assert e.value.status == 5
    h = host(ctx, name, "one", 1)
    want = h.assign_and_prove(tmpl)
    assert h.assign_and_prove(rep) == want == h.upload_proof()
    assert rep.verify(h.state, h.coms, want[0]) == 0
    rep.free(); tmpl.free()


def test_merkle_three_items(ctx):
    tmpl = template(ctx, "merkle3")
    rep, counts = launches(ctx, lambda: tmpl.repeat(3))
    assert counts == {"k_repeat_colptr": 1, "k_repeat_entries": 1, "k_repeat_coef": 1}, counts
    h = host(ctx, "merkle3", "items", 3)
    assert (rep.n, rep.m, rep.n_params) == (h.inst.n, h.inst.m, 3) == (11664, 9, 3) and h.N == 16384
    assert len(set(h.params)) == 3, "a root of its own per item"
    _, counts = launches(ctx, lambda: rep.assign(h.inst.v, h.params))
    assert counts.get("k_witness_eval_repeat") == 3 and "k_witness_eval" not in counts, counts       # one launch per level of the SOURCE
    got = rep.prove(h.state, h.inst.v_blinding, SEED)
    assert got == h.oracle_proof(), "the repeat and the oracle on the host assembly give different proofs"
    assert h.oracle_verify(got[0]) == 0
    assert rep.verify(h.state, h.coms, got[0]) == 0
    assert ctx.verify_flat(h.inst, h.state, h.coms, got[0]) == 0
    assert ctx.verify_batch([(rep, h.state, h.coms, got[0]), (h.inst, h.state, h.coms, got[0])])[0] == [0, 0]
    # item 1's root altered: the proof does not depend on constants, the statement the handle checks does
    bad = list(h.params); bad[1] = sc(int.from_bytes(bad[1], "little") + 1)
    rep.assign(h.inst.v, bad)
    assert rep.prove(h.state, h.inst.v_blinding, SEED) == got
    assert rep.verify(h.state, h.coms, got[0]) == 3                           # BPG_ERR_VERIFICATION
    rep.assign(h.inst.v, h.params)
    assert rep.verify(h.state, h.coms, got[0]) == 0
    # the source was left alone: it still proves its own witness
    one = host(ctx, "merkle3", "tmpl", 1)
    assert tmpl.prove(one.state, one.inst.v_blinding, SEED) == one.upload_proof()
    rep.free(); tmpl.free()


def bounds_host(ctx, tag, K, bad_item=None):
    t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
    a = (1 << 8) + 5                                                          # a + b = max - min holds, the 8-bit range proof of a does not
    for k in range(K):
        bounds8_item(p, tag, k, [sc(7), sc(a), sc(255 - a)] if k == bad_item else None)
    return Host(ctx, p, t, [])


def test_bounds_check_sixty_five_items(ctx):
    tmpl = template(ctx, "bounds8")
    rep = tmpl.repeat(65)
    h = bounds_host(ctx, "items", 65)
    assert (rep.n, rep.m, rep.n_params) == (h.inst.n, h.inst.m, 0) == (1040, 195, 0) and h.N == 2048
    _, counts = launches(ctx, lambda: rep.assign(h.inst.v))
    assert counts.get("k_witness_eval_repeat") == 1 and "k_witness_eval" not in counts, counts
    got = rep.prove(h.state, h.inst.v_blinding, SEED)
    assert got == h.oracle_proof()
    assert h.oracle_verify(got[0]) == 0 and rep.verify(h.state, h.coms, got[0]) == 0
    # one out-of-range value, in item 64 alone: the host's witness, the host's bytes, and a proof nobody accepts
    bad = bounds_host(ctx, "items", 65, bad_item=64)
    got = bad.assign_and_prove(rep)
    assert got == bad.upload_proof()
    assert rep.verify(bad.state, bad.coms, got[0]) == 3
    assert ctx.verify_flat(bad.inst, bad.state, bad.coms, got[0]) == 3
    assert bad.oracle_verify(got[0]) != 0
    rep.free(); tmpl.free()


def test_reassignment_drops_what_belonged_to_the_previous_witness(monkeypatch):
    """a second assign with other values: the oracle's bytes for THOSE values.  BPG_MERGE=1 and BPG_TT_ORIG_LG=0 put the proof on the path that groups equal
    scalars once per resident witness (bit vectors: large groups); a set that survived the assign would give a wrong A_I without any error."""
    monkeypatch.setenv("BPG_MERGE", "1"); monkeypatch.setenv("BPG_TT_ORIG_LG", "0")
    ctx = bpg.Context(0)
    ctx.gens_ensure(256)
    tmpl = template(ctx, "bounds8")
    rep = tmpl.repeat(9)
    first, second = bounds_host(ctx, "first", 9), bounds_host(ctx, "second", 9)
    assert first.inst.v != second.inst.v and first.N == 256
    assert first.assign_and_prove(rep) == first.oracle_proof()
    assert ctx.schedule()["merge_equal"] == 1 and ctx.schedule()["merged_skipped_last"] > 0, "this path must really build merge sets"
    assert rep.prove(first.state, first.inst.v_blinding, SEED) == first.upload_proof()          # ... again, with this witness's sets in place
    assert second.assign_and_prove(rep) == second.oracle_proof()
    assert first.assign_and_prove(rep) == first.upload_proof()
    rep.free(); tmpl.free(); ctx.close()


def test_the_source_may_be_freed_first(ctx):
    tmpl = template(ctx, "set3")
    rep = tmpl.repeat(5)
    tmpl.free()
    h = host(ctx, "set3", "life", 5)
    assert (rep.n, rep.m) == (30, 30) == (h.inst.n, h.inst.m)
    got = h.assign_and_prove(rep)
    assert got == h.oracle_proof()
    assert rep.verify(h.state, h.coms, got[0]) == 0 and h.oracle_verify(got[0]) == 0
    rep.free()
    rep.free()                                                                # (the binding's free is idempotent)


def test_template_batch_takes_the_fallback(ctx):
    """a repeat keeps no host rows: bpg_r1cs_prove_template_batch proves its items by assign + prove_resident, one at a time"""
    tmpl = template(ctx, "set3")
    rep = tmpl.repeat(2)
    hs = [host(ctx, "set3", "batch-%d" % i, 2) for i in range(2)]
    want = [h.assign_and_prove(rep) for h in hs]
    assert want[0] == hs[0].upload_proof()
    res, counts = launches(ctx, lambda: rep.prove_batch([(h.inst.v, h.params, h.state, h.inst.v_blinding, SEED, 0) for h in hs]))
    assert res == want
    assert "k_witness_eval_batch" not in counts and counts.get("k_witness_eval_repeat") == 2, counts    # one level, two items of the batch
    with pytest.raises(bpg.BpgError) as e:                                   # no witness afterwards, as documented for any template batch
        rep.prove(hs[0].state, hs[0].inst.v_blinding, SEED)
    assert e.value.status == 5
    rep.free(); tmpl.free()


def test_refusals_launch_nothing(ctx):
    tmpl = template(ctx, "set3")
    rep = tmpl.repeat(2)
    h = host(ctx, "set3", "plain", 1)
    plain = ctx.upload(h.inst)

    def attempts():
        out = []
        for c, count in ((tmpl, 0), (rep, 2), (plain, 2), (tmpl, 1 << 25), (tmpl, (1 << 64) - 1)):
            with pytest.raises(bpg.BpgError) as e:
                c.repeat(count)
            out.append((e.value.status, str(e.value)))
        return out
    res, counts = launches(ctx, attempts)
    assert counts == {}, counts
    assert [s for s, _ in res] == [4] * 5
    for (_, msg), word in zip(res, ("at least 1", "itself a repeat", "not a template", "too many", "too many")):
        assert word in msg, msg
    # arguments of assign on the repeat: count x m values, count x n_params constants
    for vals, params in ((h.inst.v, []), (h.inst.v * 2, [bytes(32)])):
        with pytest.raises((bpg.BpgError, ValueError)) as e:
            rep.assign(vals, params)
        assert not isinstance(e.value, bpg.BpgError) or e.value.status == 4
    plain.free(); rep.free(); tmpl.free()
