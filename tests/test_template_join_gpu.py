"""Templates joined on the GPU (bpg_r1cs_template_join): ONE proof for a mixed statement - some range checks AND some set memberships AND some Merkle
openings - without a host assembly of the conjunction.

The yardstick is the CPU oracle on the EXISTING host assembly - one prover that commits and assembles the same gadget code part by part, item by item
(`mixed_assembly` of tests/test_template_join_host.py): the join, built on the device from templates of ONE item each and assigned the items' values, must give
the oracle's proof bytes for that assembly, and the oracle's verifier, the GPU verifier on the host assembly and the GPU verifier on the joined handle judge
the proofs.  The join is never compared with itself.

Sizes: the mixed statement [(set3, 2), (bounds8, 65), (merkle3, 2)] has n' = 8,828 (N' = 2^14), three schedule levels (merkle3's), a parameter per Merkle
item, bit hints in every bounds8 item and 65 of them - one more than a block of the lane map holds; smaller lists wherever they will do."""
import pytest
import bulletproofs_gadgets_amd as bpg
from test_template_host import StubProver
from test_template_repeat_host import CIRCUITS, assemble, bounds8_item, sc
from test_template_repeat_gpu import Host, SEED, launches, template
from test_template_join_host import MIXED, merkle3_checkpoint_values, mixed_assembly

pytestmark = pytest.mark.gpu
JOIN_KERNELS = {"k_join_colptr", "k_join_entries", "k_join_coef"}
BAD = [sc(7), sc((1 << 8) + 5), sc(255 - ((1 << 8) + 5))]          # a + b = max - min holds; the 8-bit range proofs of a and of b < 0 do not


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(16384)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tmpls(ctx):
    """the resident templates, ONE item each; merkle3ck: merkle3 with the digests of its two nodes as checkpoints"""
    out = {name: template(ctx, name) for name in CIRCUITS}
    p, _, rows = assemble("merkle3", "tmpl", 1, prover_cls=bpg.Prover, ctx=ctx)
    out["merkle3ck"] = p.template(ctx, param_rows=rows, checkpoints=[var for var, _, last in p.noted() if last])
    yield out
    for t in out.values():
        t.free()


def host(ctx, parts, tag, bad=None):
    """the host assembly of the part list (a Host of tests/test_template_repeat_gpu.py); bad = (part, item): that bounds8 item holds an out-of-range value"""
    t = bpg.Transcript(b"MixedStatement")
    p = bpg.Prover(ctx, t)
    rows = []
    for k, (name, count) in enumerate(parts):
        for i in range(count):
            if bad == (k, i):
                rows += bounds8_item(p, "%s-part%d" % (tag, k), i, BAD)
            else:
                rows += CIRCUITS[name.replace("ck", "")][0](p, "%s-part%d" % (tag, k), i)
    return Host(ctx, p, t, rows)


def join(ctx, tmpls, parts):
    return ctx.join([(tmpls[name], count) for name, count in parts])


def checkpoint_values(h, layout, part):
    """the checkpoint values of a merkle3 part of host assembly h, item-major, from the committed leaves alone"""
    out = []
    for k in range(layout[part]["count"]):
        at = 32 * (layout[part]["base_m"] + 3 * k)
        out += merkle3_checkpoint_values(h.inst.v[at:at + 96])
    return out


def test_mixed_statement(ctx, tmpls):
    j, counts = launches(ctx, lambda: join(ctx, tmpls, MIXED))
    assert set(counts) <= JOIN_KERNELS and counts["k_join_colptr"] == counts["k_join_entries"] == 3, counts     # once per part, nothing else
    h = host(ctx, MIXED, "items")
    assert (j.n, j.m, j.n_params, j.q) == (h.inst.n, h.inst.m, 2, h.inst.q) and j.n == 8828 and h.N == 16384
    assert [(p["n"], p["count"], p["base_n"]) for p in j.layout] == [(6, 2, 0), (16, 65, 12), (3888, 2, 1052)]
    assert len(set(h.params)) == 2, "a root of its own per Merkle item"
    with pytest.raises(bpg.BpgError) as e:                                   # it starts without a witness, though the sources hold one each
        j.prove(h.state, h.inst.v_blinding, SEED)
    assert e.value.status == 5
    _, counts = launches(ctx, lambda: j.assign(h.inst.v, h.params))
    assert counts.get("k_witness_eval_join") == 3, counts                    # the MOST levels any part has - not the sum over the parts (1 + 1 + 3)
    assert "k_witness_eval" not in counts and "k_witness_eval_repeat" not in counts and "k_witness_ck_verify_join" not in counts, counts
    got = j.prove(h.state, h.inst.v_blinding, SEED)
    assert got == h.oracle_proof(), "the join and the oracle on the host assembly give different proofs"
    assert h.oracle_verify(got[0]) == 0
    assert j.verify(h.state, h.coms, got[0]) == 0
    assert ctx.verify_flat(h.inst, h.state, h.coms, got[0]) == 0
    assert ctx.verify_batch([(j, h.state, h.coms, got[0]), (h.inst, h.state, h.coms, got[0])])[0] == [0, 0]
    assert j.check().ok
    # the root of merkle3 item 1 altered: the proof does not depend on constants, the statement the handle checks does
    bad = list(h.params); bad[1] = sc(int.from_bytes(bad[1], "little") + 1)
    j.assign(h.inst.v, bad)
    assert j.prove(h.state, h.inst.v_blinding, SEED) == got
    assert j.verify(h.state, h.coms, got[0]) == 3                             # BPG_ERR_VERIFICATION
    j.assign(h.inst.v, h.params)
    assert j.verify(h.state, h.coms, got[0]) == 0
    # a source was left alone: it still proves its own witness
    one = Host(ctx, *assemble("merkle3", "tmpl", 1, prover_cls=bpg.Prover, ctx=ctx))
    assert tmpls["merkle3"].prove(one.state, one.inst.v_blinding, SEED) == one.upload_proof()
    j.free()


def test_order_matters(ctx, tmpls):
    got = []
    for parts in ([("merkle3", 1), ("bounds8", 3)], [("bounds8", 3), ("merkle3", 1)]):
        j = join(ctx, tmpls, parts)
        h = host(ctx, parts, "order")
        assert h.N == 4096
        got.append(h.assign_and_prove(j))
        assert got[-1] == h.oracle_proof(), parts
        assert j.verify(h.state, h.coms, got[-1][0]) == 0 and h.oracle_verify(got[-1][0]) == 0
        j.free()
    assert got[0][0] != got[1][0]


def test_one_part_is_the_repeat(ctx, tmpls):
    parts = [("bounds8", 65)]
    j = join(ctx, tmpls, parts)
    h = host(ctx, parts, "one")
    assert (j.n, j.m, j.n_params) == (1040, 195, 0) and h.N == 2048
    _, counts = launches(ctx, lambda: j.assign(h.inst.v))
    assert counts.get("k_witness_eval_join") == 1 and "k_witness_eval_repeat" not in counts, counts
    got = j.prove(h.state, h.inst.v_blinding, SEED)
    assert got == h.oracle_proof()
    assert j.verify(h.state, h.coms, got[0]) == 0
    j.free()


def test_checkpoints(ctx, tmpls):
    parts = [("bounds8", 3), ("merkle3ck", 2)]
    j = join(ctx, tmpls, parts)
    plain = join(ctx, tmpls, [("bounds8", 3), ("merkle3", 2)])
    h = host(ctx, parts, "ck")
    assert (j.n_ck, plain.n_ck) == (4, 0) and [p["base_n_ck"] for p in j.layout] == [0, 0] and j.layout[1]["n_ck"] == 2
    values = checkpoint_values(h, j.layout, 1)
    _, counts = launches(ctx, lambda: j.assign(h.inst.v, h.params, checkpoints=values))
    assert counts.get("k_witness_eval_join") == 2 and counts.get("k_witness_ck_verify_join") == 1, counts      # merkle3 alone: three levels
    assert "k_witness_ck_verify" not in counts and "k_witness_eval" not in counts, counts
    got = j.prove(h.state, h.inst.v_blinding, SEED)
    assert got == h.assign_and_prove(plain) == h.upload_proof()
    assert j.verify(h.state, h.coms, got[0]) == 0 and h.oracle_verify(got[0]) == 0
    # a wrong checkpoint in item 1 of the Merkle part: the flat index in the joined list, the place in words, and no witness afterwards
    for c in (1, 0):
        bad = list(values); bad[2 + c] = sc(int.from_bytes(bad[2 + c], "little") + 1)
        with pytest.raises(bpg.BpgError) as e:
            j.assign(h.inst.v, h.params, checkpoints=bad)
        assert e.value.status == bpg.ERR_CHECKPOINT_MISMATCH and e.value.first_mismatch == 2 + c and e.value.place == (1, 1, c)
        assert "checkpoint %d of item 1 of part 1" % c in str(e.value), str(e.value)
        with pytest.raises(bpg.BpgError) as e:
            j.prove(h.state, h.inst.v_blinding, SEED)
        assert e.value.status == 5                                            # BPG_ERR_MISSING_ASSIGNMENT
    with pytest.raises(bpg.BpgError) as e:                                   # plain assign on a join with a checkpointed part
        j.assign(h.inst.v, h.params)
    assert e.value.status == 4 and "checkpoints" in str(e.value)
    j.assign(h.inst.v, h.params, checkpoints=values)
    assert j.prove(h.state, h.inst.v_blinding, SEED) == got
    j.free(); plain.free()


def test_check_names_the_part_and_the_item(ctx, tmpls):
    j = join(ctx, tmpls, MIXED)
    bad = host(ctx, MIXED, "items", bad=(1, 64))
    got = bad.assign_and_prove(j)
    rep = j.check()
    assert rep == bpg.test_check_host(bad.inst) and not rep.ok
    # the row of the template that an out-of-range value breaks, from ONE such item assembled alone on the host
    p = StubProver(None, bpg.Transcript(b"BoundsCheck"))
    bounds8_item(p, "alone", 0, BAD)
    alone = bpg.test_check_host(p.instance())
    assert alone.bad_rows == len(alone.rows) == 2 and alone.bad_multipliers == 0           # the range proofs of a and of b = max - min - a < 0: one row each
    assert rep.parts(j.layout) == [(1, 64, r) for r in alone.rows] and rep.bad_rows == 2 and rep.bad_multipliers == 0 and rep.multiplier_part(j.layout) is None
    assert got == bad.upload_proof()
    assert j.verify(bad.state, bad.coms, got[0]) == 3
    assert ctx.verify_flat(bad.inst, bad.state, bad.coms, got[0]) == 3
    assert bad.oracle_verify(got[0]) != 0
    j.free()


def test_sources_may_be_freed_first_and_nothing_is_left_behind(ctx):
    parts = [("set3", 2), ("bounds8", 3), ("set3", 1)]
    hs = [host(ctx, parts, "life-%d" % i) for i in range(2)]
    want = [h.upload_proof() for h in hs]

    def cycle():
        own = {name: template(ctx, name) for name in ("set3", "bounds8")}
        j = join(ctx, own, parts)
        for t in own.values():
            t.free()                                                          # every source is gone before the first assign
        assert [h.assign_and_prove(j) for h in hs] == want
        assert j.verify(hs[1].state, hs[1].coms, want[1][0]) == 0
        # a join keeps no host rows: bpg_r1cs_prove_template_batch proves its items by assign + prove_resident, one at a time
        res, counts = launches(ctx, lambda: j.prove_batch([(h.inst.v, h.params, h.state, h.inst.v_blinding, SEED, 0) for h in hs]))
        assert res == want
        assert "k_witness_eval_batch" not in counts and counts.get("k_witness_eval_join") == 2, counts        # one level, two items of the batch
        with pytest.raises(bpg.BpgError) as e:                               # no witness afterwards, as documented for any template batch
            j.prove(hs[0].state, hs[0].inst.v_blinding, SEED)
        assert e.value.status == 5
        j.free()
        j.free()                                                              # (the binding's free is idempotent)
    assert hs[0].oracle_proof() == want[0]
    cycle()                                                                   # the context's own staging buffers grow once
    start = bpg.live_resources()
    cycle()
    assert bpg.live_resources() == start


def test_reassignment_drops_what_belonged_to_the_previous_witness(monkeypatch):
    """a second assign with other values: the host upload's bytes for THOSE values.  BPG_MERGE=1 and BPG_TT_ORIG_LG=0 put the proof on the path that groups equal
    scalars once per resident witness (bit vectors: large groups); a set that survived the assign would give a wrong A_I without any error."""
    monkeypatch.setenv("BPG_MERGE", "1"); monkeypatch.setenv("BPG_TT_ORIG_LG", "0")
    ctx = bpg.Context(0)
    ctx.gens_ensure(256)
    own = {name: template(ctx, name) for name in ("set3", "bounds8")}
    parts = [("bounds8", 8), ("set3", 2)]
    j = join(ctx, own, parts)
    first, second = host(ctx, parts, "first"), host(ctx, parts, "second")
    assert first.inst.v != second.inst.v and first.N == 256
    assert first.assign_and_prove(j) == first.oracle_proof()
    assert ctx.schedule()["merge_equal"] == 1 and ctx.schedule()["merged_skipped_last"] > 0, "this path must really build merge sets"
    assert j.prove(first.state, first.inst.v_blinding, SEED) == first.upload_proof()            # ... again, with this witness's sets in place
    assert second.assign_and_prove(j) == second.oracle_proof()
    assert first.assign_and_prove(j) == first.upload_proof()
    j.free()
    for t in own.values():
        t.free()
    ctx.close()


def test_refusals_launch_nothing(ctx, tmpls):
    rep = tmpls["set3"].repeat(2)
    jn = join(ctx, tmpls, [("set3", 1), ("bounds8", 1)])
    h = host(ctx, [("set3", 1)], "plain")
    plain = ctx.upload(h.inst)
    good = (tmpls["set3"], 1)

    def attempts():
        out = []
        for parts in ([], [good] * 257, [good, (tmpls["bounds8"], 0)], [good, (rep, 2)], [good, good, (jn, 1)], [good, (plain, 2)],
                      [good, (tmpls["bounds8"], 1 << 23)], [(tmpls["bounds8"], 1 << 22), (tmpls["bounds8"], 1 << 22)], [good, (tmpls["merkle3"], (1 << 64) - 1)]):
            with pytest.raises(bpg.BpgError) as e:
                ctx.join(parts)
            out.append((e.value.status, str(e.value)))
        return out
    res, counts = launches(ctx, attempts)
    assert counts == {}, counts
    assert [s for s, _ in res] == [4] * len(res)
    for (_, msg), word in zip(res, ("at least 1", "at most 256", "part 1: count must be at least 1", "part 1: the circuit is itself a repeat",
                                    "part 2: the circuit is itself a join", "part 1: the circuit is not a template", "part 1: the joined multipliers",
                                    "part 1: the joined multipliers", "part 1: the joined multipliers")):
        assert word in msg, msg
    # a join is no source of a repeat (its program is its parts'): refused, and so is check_batch, which repeats its template
    def repeats():
        out = []
        for call in (lambda: jn.repeat(2), lambda: jn.repeat(1), lambda: jn.check_batch([(h.inst.v, [])])):
            with pytest.raises(bpg.BpgError) as e:
                call()
            out.append((e.value.status, str(e.value)))
        return out
    res, counts = launches(ctx, repeats)
    assert counts == {}, counts
    assert all(st == 4 and "the circuit is a join" in msg and "larger counts" in msg for st, msg in res), res
    # arguments of assign on the join: the concatenated values and constants
    for vals, params in ((h.inst.v, []), (h.inst.v * 2, [bytes(32)])):
        with pytest.raises((bpg.BpgError, ValueError)) as e:
            jn.assign(vals, params)
        assert not isinstance(e.value, bpg.BpgError) or e.value.status == 4
    plain.free(); jn.free(); rep.free()
