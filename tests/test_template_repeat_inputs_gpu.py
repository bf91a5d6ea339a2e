"""Public inputs through repeat and join on the GPU (bpg_r1cs_template_repeat_inputs, bpg_r1cs_template_join_inputs, bpg_r1cs_set_inputs, k_input_slots_join):
K statements against K different public values as ONE proof.  A resident template with inputs - made from one item of another seed - is repeated or joined
on the device, assigned K witnesses with K sets of public values, and must prove exactly what Prover.prove gives on ONE FRESH HOST ASSEMBLY of the K
statements with every public value baked in as a constant (repeat_inputs_cases.Assembly, as_inputs=False): proof bytes and transcript state, never compared
with a template.  verify_resident, check() and the CPU oracle's verifier on the verifier-side assembly judge the proofs.  Everything stays at N <= 2048.

Run as a script (`python tests/test_template_repeat_inputs_gpu.py leak`) the file runs a repeat, a join and set_inputs in a process of its own, frees
everything and prints the census of what the process still holds (bpg_test_live_resources)."""
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
import repeat_inputs_cases as RC
from template_inputs_cases import sc, rng, L

pytestmark = pytest.mark.gpu
MISSING, MISMATCH = 5, bpg.ERR_CHECKPOINT_MISMATCH


def pow2(n):
    return 1 << max(n - 1, 0).bit_length()


class Baked:
    """ONE fresh host assembly of all items with the public values as constants, proved by Prover.prove: the yardstick"""
    def __init__(self, ctx, parts, tag):
        self.parts, self.tag = parts, tag
        self.a = a = RC.Assembly(parts, False, prover_cls=bpg.Prover, ctx=ctx, tag=tag)
        self.inst = a.instance()
        self.state = a.transcript.state                     # after the commitments, before the proof
        self.coms = b"".join(a.commitments)
        self.proof = a.prover.prove(pow2(self.inst.n), rng(tag))
        self.state_after = a.transcript.state
        self.inputs, self.params, self.cks = a.inputs, a.params, a.ck_values

    def assign(self, circuit, inputs=None, cks=None):
        circuit.assign(self.inst.v, self.params, checkpoints=(self.cks if cks is None else cks) or None, inputs=self.inputs if inputs is None else inputs)

    def prove_on(self, circuit):
        return circuit.prove(self.state, self.inst.v_blinding, rng(self.tag))


def device_template(ctx, name, checkpoints=False):
    a = RC.template_of(name, prover_cls=bpg.Prover, ctx=ctx)
    cks = [v for v, _, last in a.prover.noted() if last] if checkpoints else []
    return a.prover.template(ctx, checkpoints=cks)


def args_of(name, count, first=0):
    return list(range(first, first + count)) if isinstance(name, tuple) else RC.ARGS[name][first:first + count]


def launches(ctx, call):
    ctx.profile_set(2)
    res = call()
    rep = ctx.profile_report()
    ctx.profile_set(0)
    names = ("k_input_slots_join", "k_input_slots", "k_witness_eval_repeat", "k_witness_eval_join", "k_witness_eval", "k_witness_eval_batch")
    return res, {k: rep.get(k, {"count": 0})["count"] for k in names}


def levels_of(name, checkpoints=False):
    """schedule levels of the template, from the host's own planner"""
    inst, prog, hints, cks, n_in = RC.template_parts(RC.template_of(name))
    cs, cp = inst.cstruct(), prog.cstruct()
    ch = hints.cstruct() if len(hints) else None
    ck = bpg._checkpoints_cstruct(cks if checkpoints else [])
    out = C.create_string_buffer(1 << 20)
    assert bpg.lib().bpg_test_template_schedule_inputs(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck), C.c_uint64(n_in), out,
                                                       C.c_uint64(1 << 20)) == 0
    return json.loads(out.value.decode())["levels"]


def _child():
    ctx = bpg.Context(0)
    ctx.gens_ensure(1024)
    lt, ne = device_template(ctx, "less_than"), device_template(ctx, "inequality")
    rep = lt.repeat_inputs(2)
    joined = ctx.join_inputs([(ne, 2), (lt, 1)])
    lt.free(); ne.free()
    b = Baked(ctx, [("less_than", args_of("less_than", 2))], "leak repeat")
    b.assign(rep)
    ok = b.prove_on(rep) == (b.proof, b.state_after)
    rep.set_inputs(b.inputs)
    ok = ok and rep.verify(b.state, b.coms, b.proof) == 0
    j = Baked(ctx, [("inequality", args_of("inequality", 2)), ("less_than", args_of("less_than", 1))], "leak join")
    j.assign(joined)
    ok = ok and j.prove_on(joined) == (j.proof, j.state_after)
    with_open = bpg.live_resources()
    rep.free(); joined.free(); ctx.close()
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


def judged(ctx, gens, circuit, b):
    """assign + prove on the repeat or join against the baked assembly, then every judge"""
    b.assign(circuit)
    assert b.prove_on(circuit) == (b.proof, b.state_after), "%s: proof or transcript state differs from Prover.prove on the host assembly with constants" % b.tag
    assert circuit.verify(b.state, b.coms, b.proof) == 0 and circuit.check().ok, b.tag
    assert ctx.verify_batch([(circuit, b.state, b.coms, b.proof)])[0] == [0], "%s: verify_batch with the circuit as one item" % b.tag
    if all(isinstance(n, str) for n, _ in b.parts):         # gadgets have a verifier-side assembly; random shapes are judged on the prover's rows
        v = RC.replay(b.parts, b.a.commitments)
        assert O.verify(gens, v.transcript.state, to_oracle(v.instance()), b.coms, b.proof) == 0, "%s: the oracle verifier rejected the proof" % b.tag
    else:
        assert O.verify(gens, b.state, to_oracle(b.inst), b.coms, b.proof) == 0, "%s: the oracle verifier rejected the proof" % b.tag


# ------------------------------------------------------------------------------------------------ 1. the repeat
REPEATS = [("inequality", 1), ("inequality", 2), ("inequality", 3), ("set4", 1), ("set4", 2), ("set4", 3), ("less_than", 1), ("less_than", 2), ("less_than", 3)]
REPEATS += [(("random", s), 3) for s in RC.RANDOM_SEEDS.values()]


@pytest.mark.parametrize("name, K", REPEATS, ids=lambda x: x if isinstance(x, (str, int)) else "%s%d" % x)
def test_repeat_proves_the_host_assembly_with_constants(ctx, gens, name, K):
    tmpl = device_template(ctx, name)
    rep = tmpl.repeat_inputs(K)
    tmpl.free()                                             # the source is freed before the repeat is first used
    try:
        assert (rep.n, rep.m, rep.n_inputs) == (K * tmpl.n, K * tmpl.m, K * tmpl.n_inputs) and rep.n_inputs > 0 and pow2(rep.n) <= 2048
        judged(ctx, gens, rep, Baked(ctx, [(name, args_of(name, K))], "repeat %s %d" % (name, K)))
    finally:
        rep.free()


def test_repeat_of_65_crosses_the_block_of_64_items(ctx):
    """K = 65 on Inequality (n = 195, N = 256): the second block of k_witness_eval_repeat holds one item.  a_L, a_R, a_O against the host hook through check(),
    the proof against the baked assembly"""
    K = 65
    args = [(1000 + 3 * k, 7 * k + (2**130 if k % 5 == 0 else 0)) for k in range(K)]
    tmpl = device_template(ctx, "inequality")
    rep = tmpl.repeat_inputs(K)
    tmpl.free()
    try:
        b = Baked(ctx, [("inequality", args)], "repeat 65")
        tinst, prog, hints, cks, n_in = RC.template_parts(RC.template_of("inequality"))
        aL, aR, aO, _ = bpg.test_template_eval_repeat_inputs(tinst, prog, hints, cks, n_in, K, b.inst.v, None, b.inputs)
        assert (aL, aR, aO) == (b.inst.aL, b.inst.aR, b.inst.aO)
        (_, n) = launches(ctx, lambda: b.assign(rep))
        assert n["k_input_slots_join"] == 1 and n["k_witness_eval_repeat"] == levels_of("inequality") and n["k_witness_eval"] == n["k_input_slots"] == 0, n
        rpt = rep.check()
        assert rpt.ok and rpt == ctx.check_flat(b.inst), rpt       # the device's vectors satisfy the rows the host's vectors satisfy: the same witness
        assert b.prove_on(rep) == (b.proof, b.state_after)
        assert rep.verify(b.state, b.coms, b.proof) == 0
        # one item's input off by one: exactly that item's rows break
        bad = list(b.inputs); bad[64] = sc(int.from_bytes(bad[64], "little") + 1)
        b.assign(rep, inputs=bad)
        assert {r // tmpl.q for r in rep.check(None, 64).rows} == {64}
    finally:
        rep.free()


def test_repeat_launch_counts(ctx):
    tmpl = device_template(ctx, "less_than")
    rep = tmpl.repeat_inputs(3)
    try:
        b = Baked(ctx, [("less_than", args_of("less_than", 3))], "repeat launches")
        levels = levels_of("less_than")
        for _ in range(2):                                   # per assign, whichever comes first
            _, n = launches(ctx, lambda: b.assign(rep))
            assert n == {"k_input_slots_join": 1, "k_input_slots": 0, "k_witness_eval_repeat": levels, "k_witness_eval_join": 0, "k_witness_eval": 0, "k_witness_eval_batch": 0}, n
        _, n = launches(ctx, lambda: rep.set_inputs(b.inputs))
        assert n["k_input_slots_join"] == 1 and sum(n.values()) == 1, n
        _, n = launches(ctx, lambda: tmpl.set_inputs(b.inputs[:1]))      # a single template keeps its own kernel
        assert n["k_input_slots"] == 1 and sum(n.values()) == 1, n
    finally:
        rep.free(); tmpl.free()


# ------------------------------------------------------------------------------------------------ 2. the join
JOINS = {
    "with2_without3_with1": [("inequality", 2), (("plain", 2), 3), ("set4", 1)],
    "same_template_twice": [(("random", 1), 2), ("inequality", 1), (("random", 1), 1)],
    "a_part_with_m_0": [("set4", 1), (("random", 50), 2), (("random", 4), 2)],
}


def join_of(ctx, spec, tag, checkpoints=()):
    """(the join, its baked assembly): one resident template per distinct name, freed before the join is used"""
    made, seen, parts = {}, {}, []
    for name, count in spec:
        if name not in made:
            if isinstance(name, tuple) and name[0] == "plain":
                a = RC.Assembly([(name, [1000 + name[1]])], True, prover_cls=bpg.Prover, ctx=ctx, tag="tmpl")
                made[name] = a.prover.template(ctx)
            else:
                made[name] = device_template(ctx, name, checkpoints=name in checkpoints)
        parts.append((name, args_of(name, count, seen.get(name, 0))))
        seen[name] = seen.get(name, 0) + count
    joined = ctx.join_inputs([(made[name], count) for name, count in spec])
    for t in made.values():
        t.free()
    return joined, Baked(ctx, parts, tag), made


@pytest.mark.parametrize("join", sorted(JOINS))
def test_join_proves_the_host_assembly_with_constants(ctx, gens, join):
    joined, b, made = join_of(ctx, JOINS[join], "join " + join)
    try:
        assert joined.n_inputs == len(b.inputs) == sum(c * made[n].n_inputs for n, c in JOINS[join])
        assert [p["base_n_inputs"] for p in joined.layout] == [sum(c * made[n].n_inputs for n, c in JOINS[join][:k]) for k in range(len(JOINS[join]))]
        judged(ctx, gens, joined, b)
    finally:
        joined.free()


def test_join_launch_counts_and_checkpoint_mismatch(ctx, gens):
    """(Inequality, 2), (the Merkle node (W I) with its digest checkpointed, 1): n = 1950.  One slot launch and one k_witness_eval_join per level of the
    deepest part per assign; a wrong digest reports (part 1, item 0, checkpoint 0) and leaves no witness"""
    spec = [("inequality", 2), ("merkle_wi", 1)]
    joined, b, made = join_of(ctx, spec, "join ck", checkpoints=("merkle_wi",))
    try:
        assert joined.n_ck == 1 and joined.n_inputs == 4 and b.cks == [RC.TC.merkle_root([sc(11), sc(22)])]
        deepest = max(levels_of("inequality"), levels_of("merkle_wi", checkpoints=True))
        _, n = launches(ctx, lambda: b.assign(joined))
        assert n == {"k_input_slots_join": 1, "k_input_slots": 0, "k_witness_eval_repeat": 0, "k_witness_eval_join": deepest, "k_witness_eval": 0, "k_witness_eval_batch": 0}, n
        assert b.prove_on(joined) == (b.proof, b.state_after) and joined.verify(b.state, b.coms, b.proof) == 0 and joined.check().ok
        with pytest.raises(bpg.BpgError) as e:
            b.assign(joined, cks=[sc(12345)])
        assert e.value.status == MISMATCH and e.value.first_mismatch == 0 and e.value.place == (1, 0, 0)
        assert "checkpoint 0 of item 0 of part 1" in str(e.value)
        with pytest.raises(bpg.BpgError) as e:
            b.prove_on(joined)
        assert e.value.status == MISSING
        b.assign(joined)
        assert b.prove_on(joined) == (b.proof, b.state_after)
    finally:
        joined.free()


# ------------------------------------------------------------------------------------------------ 3. the input matters, per item; set_inputs
def test_the_input_matters_per_item(ctx):
    """item 1 of three LessThan statements is assigned the bound + 1 while its witness keeps the right bound's delta: exactly the LAST row of item 1 breaks"""
    tmpl = device_template(ctx, "less_than")
    rep = tmpl.repeat_inputs(3)
    tmpl.free()
    try:
        q = tmpl.q
        args = [RC.ARGS["less_than"][k] for k in (0, 5, 2)]      # item 1: 77 < 5000, far from 2^126 (a bound that reaches it breaks a range row as well)
        b = Baked(ctx, [("less_than", args)], "matters")
        off = list(b.inputs); off[1] = sc(int.from_bytes(off[1], "little") + 1)
        b.assign(rep, inputs=off)
        rpt = rep.check()
        assert rpt.bad_multipliers == 0 and rpt.rows == [1 * q + (q - 1)], rpt
        assert rep.verify(b.state, b.coms, b.proof) == 3      # the honest proof against the repeat under the other bound
        b.assign(rep)
        assert rep.check().ok and rep.verify(b.state, b.coms, b.proof) == 0
    finally:
        rep.free()


def test_set_inputs_is_the_verifiers_half(ctx):
    b = Baked(ctx, [("less_than", args_of("less_than", 3))], "set_inputs")
    inst, prog, hints, cks, n_in = RC.template_parts(RC.template_of("less_than"))
    shape = ctx.upload_template(inst, prog, hints, inputs=n_in)           # an instance without a witness and without values: the shape alone
    rep = shape.repeat_inputs(3)
    shape.free()
    try:
        rep.set_inputs(b.inputs)
        assert rep.verify(b.state, b.coms, b.proof) == 0
        changed = list(b.inputs); changed[2] = sc(int.from_bytes(changed[2], "little") + 1)
        rep.set_inputs(changed)
        assert rep.verify(b.state, b.coms, b.proof) == 3
        for call in (lambda: b.prove_on(rep), lambda: rep.check()):
            with pytest.raises(bpg.BpgError) as e:
                call()
            assert e.value.status == MISSING
        b.assign(rep)                                       # a later assign proves again, with the same bytes
        assert b.prove_on(rep) == (b.proof, b.state_after)
        rep.set_inputs(b.inputs)                            # ... and set_inputs takes the witness away again
        with pytest.raises(bpg.BpgError) as e:
            b.prove_on(rep)
        assert e.value.status == MISSING
        with pytest.raises(bpg.BpgError) as e:
            rep.set_inputs(b.inputs[:2])
        assert e.value.status == 4 and "n_inputs does not match" in str(e.value)
    finally:
        rep.free()
    # on a single template: set_inputs + verify is assign + verify
    one = Baked(ctx, [("less_than", args_of("less_than", 1, 5))], "set_inputs single")
    other = Baked(ctx, [("less_than", args_of("less_than", 1, 6))], "set_inputs other")
    tmpl = device_template(ctx, "less_than")
    try:
        for setter in (lambda x: x.assign(tmpl), lambda x: tmpl.set_inputs(x.inputs)):
            setter(one)
            got = (tmpl.verify(one.state, one.coms, one.proof), tmpl.verify(other.state, other.coms, other.proof))
            setter(other)
            assert got + (tmpl.verify(one.state, one.coms, one.proof), tmpl.verify(other.state, other.coms, other.proof)) == (0, 3, 3, 0)
    finally:
        tmpl.free()


# ------------------------------------------------------------------------------------------------ 4. check_batch_inputs, prove_batch_inputs on a repeat
def test_check_batch_inputs_names_the_bad_item(ctx):
    """five LessThan items against five bounds; item 3 carries the delta of another bound"""
    bounds = [9, 2**64 + 1, 2**126 - 1, 1000, 2**100]
    args = [(b - 1 - 3 * k, b) for k, b in enumerate(bounds)]
    args[3] = (args[3][0], bounds[3], bounds[3] + 1 - args[3][0])
    tmpl = device_template(ctx, "less_than")
    try:
        own = Baked(ctx, [("less_than", args_of("less_than", 1, 7))], "check_batch own")
        own.assign(tmpl)
        before = own.prove_on(tmpl)
        assert before == (own.proof, own.state_after)
        items = []
        for k, a in enumerate(args):
            one = RC.Assembly([("less_than", [a])], False, tag="check_batch %d" % k)
            items.append((one.instance().v, [], one.inputs))
        assert tmpl.check_batch_inputs(items) == [[], [], [], [tmpl.q - 1], []]
        with pytest.raises(bpg.BpgError) as e:                # the older composition keeps refusing
            tmpl.check_batch([it[:2] for it in items])
        assert e.value.status == 4 and "public inputs" in str(e.value)
        assert own.prove_on(tmpl) == before, "check_batch_inputs touched the template's own witness"
    finally:
        tmpl.free()


def test_prove_batch_inputs_on_a_repeat_goes_item_by_item(ctx):
    tmpl = device_template(ctx, "less_than")
    rep = tmpl.repeat_inputs(2)
    tmpl.free()
    try:
        bs = [Baked(ctx, [("less_than", args_of("less_than", 2, first))], "batch on repeat %d" % first) for first in (0, 2)]
        single = []
        for b in bs:
            b.assign(rep)
            single.append(b.prove_on(rep))
        items = [(b.inst.v, [], b.state, b.inst.v_blinding, rng(b.tag), 0, None, b.inputs) for b in bs]
        res, n = launches(ctx, lambda: rep.prove_batch_inputs(items))
        assert [r[:2] for r in res] == single == [(b.proof, b.state_after) for b in bs]
        assert n["k_input_slots_join"] == 2 and n["k_witness_eval_batch"] == 0 and n["k_input_slots"] == 0, n
    finally:
        rep.free()


# ------------------------------------------------------------------------------------------------ 5. one context, mixed order
def test_one_context_in_mixed_order():
    """a lockstep wave on the source, repeat_inputs, a plain 2^10 proof, assign + prove on the repeat, join_inputs + prove, the wave again - every result
    byte-exact against the baked assemblies"""
    ctx = bpg.Context(0)
    ctx.gens_ensure(1024)
    tmpl = ne = rep = joined = None
    try:
        tmpl, ne = device_template(ctx, "less_than"), device_template(ctx, "inequality")
        singles = [Baked(ctx, [("less_than", args_of("less_than", 1, k))], "mixed wave %d" % k) for k in range(3)]
        wave = [(b.inst.v, [], b.state, b.inst.v_blinding, rng(b.tag), 0, None, b.inputs) for b in singles]
        want = [(b.proof, b.state_after) for b in singles]
        res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(wave))
        assert [r[:2] for r in res] == want and n["k_witness_eval_batch"] == 1 and n["k_input_slots"] == 1, n       # 1. the lockstep wave
        rep = tmpl.repeat_inputs(2)                                                                                  # 2.
        plain = Baked(ctx, [("less_than", args_of("less_than", 2, 4))], "mixed plain")                               # 3. a plain proof at N = 2^10 (Prover.prove)
        assert pow2(plain.inst.n) == 1024 and ctx.prove_flat(plain.inst, plain.state, plain.inst.v_blinding, rng(plain.tag)) == (plain.proof, plain.state_after)
        b = Baked(ctx, [("less_than", args_of("less_than", 2, 2))], "mixed repeat")
        b.assign(rep)                                                                                                # 4.
        assert b.prove_on(rep) == (b.proof, b.state_after)
        joined = ctx.join_inputs([(tmpl, 2), (ne, 3)])                                                               # 5.
        j = Baked(ctx, [("less_than", args_of("less_than", 2, 6)), ("inequality", args_of("inequality", 3))], "mixed join")
        assert pow2(j.inst.n) == 1024
        j.assign(joined)
        assert j.prove_on(joined) == (j.proof, j.state_after) and joined.verify(j.state, j.coms, j.proof) == 0
        res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(wave))                                                # 6. the wave again
        assert [r[:2] for r in res] == want and n["k_witness_eval_batch"] == 1, n
        assert b.prove_on(rep) == (b.proof, b.state_after)       # the repeat's witness and slots stood through all of it
    finally:
        for c in (tmpl, ne, rep, joined):
            if c is not None:
                c.free()
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. refusals on the device, resources
def test_refusals_on_the_device(ctx):
    tmpl = device_template(ctx, "inequality")
    rep = tmpl.repeat_inputs(2)
    joined = ctx.join_inputs([(tmpl, 1)])
    try:
        for src, word in ((rep, "itself a repeat"), (joined, "a join")):
            with pytest.raises(bpg.BpgError) as e:
                src.repeat_inputs(2)
            assert e.value.status == 4 and word in str(e.value), str(e.value)
            with pytest.raises(bpg.BpgError) as e:
                ctx.join_inputs([(tmpl, 1), (src, 1)])
            assert e.value.status == 4 and "part 1" in str(e.value) and word in str(e.value), str(e.value)
        b = Baked(ctx, [("inequality", args_of("inequality", 2))], "refusals")
        for call in (lambda: rep.assign(b.inst.v), lambda: rep.assign(b.inst.v, checkpoints=[])):
            with pytest.raises(bpg.BpgError) as e:
                call()
            assert e.value.status == 4 and "public inputs" in str(e.value)
        with pytest.raises(bpg.BpgError) as e:                # the frozen calls keep refusing, with their messages
            tmpl.repeat(2)
        assert "a repeat carries none" in str(e.value)
        with pytest.raises(bpg.BpgError) as e:
            ctx.join([(tmpl, 2)])
        assert "a join carries none" in str(e.value)
    finally:
        rep.free(); joined.free(); tmpl.free()


def test_nothing_is_left_behind():
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "leak"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["open"][0] > 0 and out["end"] == [0] * 6, out
