"""Public inputs in circuit templates on the GPU (bpg_r1cs_upload_template_inputs, bpg_r1cs_assign_inputs, bpg_r1cs_prove_template_batch_inputs, k_input_slots):
ONE template, made from one (witness, public values) pair, is assigned other witnesses under other public values and must prove exactly what
Prover.prove gives on a FRESH HOST ASSEMBLY with those values baked in as constants (template_inputs_cases.py, as_inputs=False) - proof bytes and transcript
states, never compared with the template itself.  The CPU oracle's verifier and verify_resident judge the proofs.

Circuits: SetMembership over a public set of 4 (n = 8), Inequality with a public right-hand side (n = 3), LessThan against a public bound (n = 379,
N = 512), MerkleTree256 (W I) with a public sibling and root (n = 1944, N = 2048).

Run as a script (`python tests/test_template_inputs_gpu.py leak`) the file runs the scenarios in a process of its own, frees everything and prints the
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
import template_inputs_cases as TC
from template_inputs_cases import sc, rng, L

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
MISMATCH = bpg.ERR_CHECKPOINT_MISMATCH


def state_before(label):
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(label)
    bpg.Prover(None, t)
    return t.state


class Host:
    """a fresh host assembly WITH CONSTANTS, proved by Prover.prove: the yardstick of one (witness, public values) pair"""
    def __init__(self, ctx, case, tag):
        self.case, self.tag = case, tag
        self.inst = case.prover.instance()
        self.state = case.transcript.state                  # after the commitments, before the proof
        self.coms = b"".join(case.commitments)
        self.proof = case.prover.prove(case.gens_capacity, rng(tag))
        self.state_after = case.transcript.state


def host_of(ctx, name, k):
    return Host(ctx, TC.build(name, k, False, ctx=ctx), "%s %d" % (name, k))


def inputs_of(name, k):
    return TC.build(name, k, True, prover_cls=TC.StubProver).inputs


def lt_host(ctx, left, bound, tag, delta=None):
    return Host(ctx, TC.less_than(ctx, left, bound, False, tag=tag, delta=delta), tag)


def scenario(ctx, name):
    """one template from case 0, assigned cases 0, 1, 2 -> [(proof, state after) from the template, Host]"""
    tmpl = TC.build(name, 0, True, ctx=ctx).prover.template(ctx)
    out = []
    try:
        assert tmpl.n_inputs == len(inputs_of(name, 0)) > 0
        for k in (1, 2, 0):
            h = host_of(ctx, name, k)
            tmpl.assign(h.inst.v, inputs=inputs_of(name, k))
            out.append((tmpl.prove(h.state, h.inst.v_blinding, rng(h.tag)), tmpl.verify(h.state, h.coms, h.proof), tmpl.check().ok, h))
    finally:
        tmpl.free()
    return out


def _child():
    ctx = bpg.Context(0)
    ctx.gens_ensure(2048)
    ok = True
    for name in ("set4", "less_than"):
        ok = ok and all(got == (h.proof, h.state_after) and verdict == 0 and sat for got, verdict, sat, h in scenario(ctx, name))
    tmpl = TC.less_than(ctx, 5, 1000, True, tag="leak").prover.template(ctx)
    hs = [lt_host(ctx, 10 + k, 500 + 7 * k, "leak %d" % k) for k in range(3)]
    pre = state_before(b"LessThan")
    res = tmpl.prove_batch_inputs([(h.inst.v, [], pre, h.inst.v_blinding, rng(h.tag), 0, None, [sc(500 + 7 * k)]) for k, h in enumerate(hs)], commit=True)
    ok = ok and [r[0] for r in res] == [h.proof for h in hs]
    with_open = bpg.live_resources()
    tmpl.free(); ctx.close()
    print(json.dumps({"ok": ok, "open": [with_open[k] for k in bpg.LIVE_RESOURCE_KEYS], "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}))


if __name__ == "__main__":
    _child()
    sys.exit(0)

import oracle_lib as O
from test_template_gpu import to_oracle


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(2048)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens():
    return O.Gens(2048)


# ------------------------------------------------------------------------------------------------ 1. single proofs
@pytest.mark.parametrize("name", sorted(TC.GADGETS))
def test_single_proofs(ctx, gens, name):
    for got, verdict, sat, h in scenario(ctx, name):
        assert got[0] == h.proof, "%s: the template's proof differs from Prover.prove on the host assembly with constants" % h.tag
        assert got[1] == h.state_after, "%s: transcript state after the proof" % h.tag
        assert verdict == 0 and sat, "%s: verify_resident / check on the template" % h.tag
        v = bpg.Verifier(bpg.Transcript(h.case.label))
        h.case.replay(v)
        assert O.verify(gens, v.transcript.state, to_oracle(v.instance()), h.coms, got[0]) == 0, "%s: the oracle verifier rejected the proof" % h.tag


# ------------------------------------------------------------------------------------------------ 2. the input matters
def test_the_input_matters(ctx, gens):
    T, T2, left = 1000, 1001, 5
    tmpl = TC.less_than(ctx, 1, 2, True, tag="matters").prover.template(ctx)
    try:
        h = lt_host(ctx, left, T, "matters T")
        tmpl.assign(h.inst.v, inputs=[sc(T)])
        proof, _ = tmpl.prove(h.state, h.inst.v_blinding, rng(h.tag))
        assert proof == h.proof and tmpl.verify(h.state, h.coms, proof) == 0
        good, bad = bpg.Verifier(bpg.Transcript(b"LessThan")), bpg.Verifier(bpg.Transcript(b"LessThan"))
        h.case.replay(good, bound_=T); h.case.replay(bad, bound_=T2)
        assert good.is_valid(proof, ctx, 512) and not bad.is_valid(proof, ctx, 512)
        worse = bpg.Verifier(bpg.Transcript(b"LessThan"))
        h.case.replay(worse, bound_=T2, as_inputs_=True)                            # the verifier's own inputs resolve to its constants
        assert not worse.is_valid(proof, ctx, 512)
        assert O.verify(gens, bad.transcript.state, to_oracle(bad.instance()), h.coms, proof) != 0
        h2 = lt_host(ctx, left, T2, "matters T2")
        tmpl.assign(h2.inst.v, inputs=[sc(T2)])
        assert tmpl.verify(h.state, h.coms, proof) == 3                             # checked against the inputs of the last assign
        assert tmpl.verify(h2.state, h2.coms, h2.proof) == 0
    finally:
        tmpl.free()


# ------------------------------------------------------------------------------------------------ 3. check() sees the patched slots
def test_check_names_the_row_of_the_public_bound(ctx):
    tmpl = TC.less_than(ctx, 1, 2, True, tag="check").prover.template(ctx)
    try:
        left, T = 77, 5000
        wrong = lt_host(ctx, left, T, "check wrong", delta=T + 1 - left)            # the delta of another bound: every range holds, one row does not
        tmpl.assign(wrong.inst.v, inputs=[sc(T)])
        rep = tmpl.check()
        assert rep.bad_multipliers == 0 and rep.bad_rows == 1 and rep.rows == [tmpl.q - 1], rep      # (right - left) - delta: the last constrain() of LessThan
        assert rep == ctx.check_flat(wrong.inst)
        tmpl.assign(wrong.inst.v, inputs=[sc(T + 1)])                               # the bound that delta belongs to
        assert tmpl.check().ok
        right = lt_host(ctx, left, T, "check right")
        tmpl.assign(right.inst.v, inputs=[sc(T)])
        assert tmpl.check().ok
    finally:
        tmpl.free()


# ------------------------------------------------------------------------------------------------ 4. lockstep batches
@pytest.fixture(scope="module")
def lt5(ctx):
    """five LessThan statements with five different bounds, their host assemblies with constants, and assign + prove per item on one template"""
    tmpl = TC.less_than(ctx, 1, 2, True, tag="lt5").prover.template(ctx)
    bounds = [9, 2**64 + 1, 2**126 - 1, 1000, 2**100]
    hs = [lt_host(ctx, b - 1 - 3 * k, b, "lt5 %d" % k) for k, b in enumerate(bounds)]
    single = []
    for h, b in zip(hs, bounds):
        tmpl.assign(h.inst.v, inputs=[sc(b)])
        single.append(tmpl.prove(h.state, h.inst.v_blinding, rng(h.tag)))
    yield tmpl, bounds, hs, single
    tmpl.free()


def launches(ctx, call):
    ctx.profile_set(2)
    res = call()
    rep = ctx.profile_report()
    ctx.profile_set(0)
    return res, {k: rep.get(k, {"count": 0})["count"] for k in ("k_input_slots", "k_witness_eval_batch", "k_witness_eval", "k_bt_commit_v")}


@pytest.mark.parametrize("commit", [False, True])
def test_lockstep_batch(ctx, lt5, commit):
    tmpl, bounds, hs, single = lt5
    pre = state_before(b"LessThan")
    items = [(h.inst.v, [], pre if commit else h.state, h.inst.v_blinding, rng(h.tag), 0, None, [sc(b)]) for h, b in zip(hs, bounds)]
    res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(items, commit=commit))
    assert n["k_input_slots"] == 1 and n["k_witness_eval_batch"] == 1 and n["k_witness_eval"] == 0 and n["k_bt_commit_v"] == (1 if commit else 0), n
    for k, h in enumerate(hs):
        assert res[k][0] == single[k][0] == h.proof, "item %d: proof bytes" % k
        assert res[k][1] == single[k][1] == h.state_after, "item %d: transcript state after" % k
        if commit:
            assert res[k][2] == h.coms, "item %d: commitments" % k
    with pytest.raises(bpg.BpgError) as e:                   # afterwards the template holds no witness, as after every template batch
        tmpl.prove(hs[0].state, hs[0].inst.v_blinding, rng("x"))
    assert e.value.status == 5
    # an item without its inputs fails alone
    items[1] = items[1][:7] + (None,)
    res, st, first = tmpl.prove_batch_inputs(items, commit=commit, return_status=True)
    assert st == [0, 4, 0, 0, 0] and res[1][0] is None and [r[0] for r in res[:1] + res[2:]] == [h.proof for h in hs[:1] + hs[2:]]


@pytest.mark.parametrize("commit", [False, True])
def test_items_off_the_lockstep_path(ctx, lt5, commit):
    """expanded blinding always takes the single path: assign_inputs + prove_resident in item order, beside lockstep items of the same call"""
    tmpl, bounds, hs, single = lt5
    EXP = bpg.FLAG_EXPANDED_BLINDING
    pre = state_before(b"LessThan")
    want = []
    for k in (1, 3):
        tmpl.assign(hs[k].inst.v, inputs=[sc(bounds[k])])
        want.append(tmpl.prove(hs[k].state, hs[k].inst.v_blinding, rng(hs[k].tag), flags=EXP))
    assert want[0][0] != hs[1].proof
    flags = [0, EXP, 0, EXP, 0]
    items = [(h.inst.v, [], pre if commit else h.state, h.inst.v_blinding, rng(h.tag), f, None, [sc(b)]) for h, b, f in zip(hs, bounds, flags)]
    res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(items, commit=commit))
    assert n["k_input_slots"] == 3 and n["k_witness_eval"] == 2 and n["k_witness_eval_batch"] == 1, n       # one wave of three, two single assigns
    assert [r[:2] for r in res] == [(hs[0].proof, hs[0].state_after), want[0], (hs[2].proof, hs[2].state_after), want[1], (hs[4].proof, hs[4].state_after)]
    if commit:
        assert [r[2] for r in res] == [h.coms for h in hs]


def test_older_calls_are_refused_on_the_device_too(ctx, lt5):
    tmpl, bounds, hs, single = lt5
    h = hs[0]
    with pytest.raises(bpg.BpgError) as e:
        tmpl.assign(h.inst.v)
    assert e.value.status == 4 and "public inputs" in str(e.value)
    with pytest.raises(bpg.BpgError) as e:
        tmpl.prove_batch([(h.inst.v, [], h.state, h.inst.v_blinding, rng(h.tag), 0)])
    assert e.value.status == 4 and "public inputs" in str(e.value)
    with pytest.raises(bpg.BpgError) as e:
        tmpl.repeat(2)
    assert e.value.status == 4 and "public inputs" in str(e.value)


def test_checkpointed_merkle_batch_with_inputs(ctx):
    """(W I) with the node's digest checkpointed and sibling and root as inputs: a batch of 3, one item's checkpoint wrong - it alone reports the mismatch"""
    base = TC.build("merkle_wi", 0, True, ctx=ctx)
    ck_vars = [v for v, _, last in base.prover.noted() if last]
    assert len(ck_vars) == 1
    tmpl = base.prover.template(ctx, checkpoints=ck_vars)
    try:
        assert tmpl.n_ck == 1 and tmpl.n_inputs == 2
        hs = [host_of(ctx, "merkle_wi", k) for k in range(3)]
        cks = [[h.case.root] for h in hs]
        cks[1] = [sc(12345)]
        items = [(h.inst.v, [], h.state, h.inst.v_blinding, rng(h.tag), 0, cks[k], inputs_of("merkle_wi", k)) for k, h in enumerate(hs)]
        (res, st, first), n = launches(ctx, lambda: tmpl.prove_batch_inputs(items, return_status=True))
        assert n["k_input_slots"] == 1 and n["k_witness_eval_batch"] == 2 and n["k_witness_eval"] == 0, n      # one wave, the two levels of the checkpointed node
        assert st == [0, MISMATCH, 0] and first == [None, 0, None]
        assert res[1] == (None, hs[1].state)
        for k in (0, 2):
            assert res[k] == (hs[k].proof, hs[k].state_after), "item %d" % k
        # and one at a time: the same mismatch, the same bytes
        with pytest.raises(bpg.BpgError) as e:
            tmpl.assign(hs[1].inst.v, checkpoints=cks[1], inputs=inputs_of("merkle_wi", 1))
        assert e.value.status == MISMATCH and e.value.first_mismatch == 0
        tmpl.assign(hs[1].inst.v, checkpoints=[hs[1].case.root], inputs=inputs_of("merkle_wi", 1))
        assert tmpl.prove(hs[1].state, hs[1].inst.v_blinding, rng(hs[1].tag)) == (hs[1].proof, hs[1].state_after)
    finally:
        tmpl.free()


# ------------------------------------------------------------------------------------------------ 5. no leak
def test_nothing_is_left_behind():
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "leak"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["open"][0] > 0 and out["end"] == [0] * 6, out
