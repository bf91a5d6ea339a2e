"""Gated variables without a GPU (bpg_prover_gate, bpg_r1cs_upload_template_gated): the host model, the plan, the packer and the interpreter compiled for the
host (the _gated test hooks), the derived coefficient slots and every refusal.

The yardstick is never the gated circuit: it is a FRESH HOST ASSEMBLY of the same statement with the public values baked in as constants (gate_cases.py:
hand10(gated=False); for Merkle paths the reference gadget MerkleTree256 over the index's own pattern), which knows nothing of inputs or gates.  One template
is made from one (witness, inputs) pair and evaluated under others."""
import ctypes as C
import json

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import gate_cases as G
from gate_cases import sc, L, StubProver
from test_template_inputs_host import meaning, meaning_of, witness, schedule_inputs, packed_inputs, hand8, INPUT_VECTORS, HAND_VALUES, _err

FAKE = C.c_void_p(1)
NONE = 2**64 - 1
LC = bpg.LinearCombination


def template_of(case):
    """(instance that keeps input and gated terms, program, hints, input values, gate table)"""
    inst, values = case.prover.template_instance()
    prog, hints = case.prover.witness_program(hints=True)
    assert values == case.inputs
    return inst, prog, hints, values, case.prover.gates()


def _views(tmpl, ck_vars=()):
    inst, prog, hints, _, gates = tmpl
    cs, cp = inst.cstruct(), prog.cstruct()
    ch = hints.cstruct() if hints is not None and len(hints) else None
    ck = bpg._checkpoints_cstruct(list(ck_vars))
    gs, keep = bpg._gates_cstruct(gates)
    return cs, cp, C.byref(ch) if ch is not None else None, ck, gs, (ch, keep)


def eval_gated(tmpl, v, inputs, ck_vars=(), ck_values=None, expect=0):
    inst = tmpl[0]
    cs, cp, ch, ck, gs, keep = _views(tmpl, ck_vars)
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    first = C.c_uint64(12345)
    st = bpg.lib().bpg_test_template_eval_gated(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(inputs)), C.byref(gs), v,
                                                b"".join(ck_values) if ck_values else None, b"".join(inputs), *out, C.byref(first))
    assert st == expect, _err()
    return out[0].raw, out[1].raw, out[2].raw, None if first.value == NONE else first.value


def eval_batch_gated(tmpl, vs, inputs, ck_vars=(), ck_values=None):
    inst = tmpl[0]
    K, N = len(vs), 1 << (inst.n - 1).bit_length()
    cs, cp, ch, ck, gs, keep = _views(tmpl, ck_vars)
    out = [C.create_string_buffer(32 * N * K) for _ in range(3)]
    first = (C.c_uint64 * max(K, 1))(*[12345] * max(K, 1))
    st = bpg.lib().bpg_test_template_eval_batch_gated(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(inputs[0])), C.byref(gs), C.c_uint64(K), b"".join(vs),
                                                      b"".join(b"".join(x) for x in ck_values) if ck_values else None, b"".join(b"".join(x) for x in inputs), *out, first)
    assert st == 0, _err()
    res = []
    for k in range(K):
        item = tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out)
        assert all(x[32 * inst.n:] == bytes(32 * (N - inst.n)) for x in item), "item %d: padding rows are not zero" % k
        res.append(tuple(x[:32 * inst.n] for x in item))
    return res, [None if first[k] == NONE else first[k] for k in range(K)]


def gated_instance(tmpl, inputs):
    """bpg_test_template_gated_instance -> (row_ptr, term_var, term_coef, coef bytes): the resident rows as an assign of `inputs` leaves them"""
    inst, prog = tmpl[0], tmpl[1]
    cs, cp, ch, ck, gs, keep = _views(tmpl)
    rows, terms, coefs = inst.q + 1, inst.nnz + 8, inst.ncoef + inst.nnz + 8
    rp, tv, tc = np.zeros(rows, np.uint64), np.zeros(terms, np.uint32), np.zeros(terms, np.uint32)
    coef = C.create_string_buffer(32 * coefs)
    nnz, ncoef = C.c_uint64(), C.c_uint64()
    st = bpg.lib().bpg_test_template_gated_instance(C.byref(cs), C.byref(cp), ch, C.c_uint64(len(inputs)), C.byref(gs), None, b"".join(inputs),
                                                    C.c_void_p(rp.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data), C.c_void_p(tc.ctypes.data), C.c_uint64(terms),
                                                    coef, C.c_uint64(coefs), C.byref(nnz), C.byref(ncoef))
    assert st == 0, _err()
    return rp, tv[:nnz.value], tc[:nnz.value], coef.raw[:32 * ncoef.value]


def schedule_gated(tmpl, ck_vars=(), raw=False, expect=0, n_in=None):
    cs, cp, ch, ck, gs, keep = _views(tmpl, ck_vars)
    buf = C.create_string_buffer(1 << 20)
    st = bpg.lib().bpg_test_template_schedule_gated(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(tmpl[3]) if n_in is None else n_in), C.byref(gs), buf,
                                                    C.c_uint64(len(buf)))
    assert st == expect, _err()
    return buf.value if raw or st else json.loads(buf.value.decode())


def packed_gated(tmpl, ck_vars=(), gates=True):
    cs, cp, ch, ck, gs, keep = _views(tmpl, ck_vars)
    words = C.c_uint64()
    args = (C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(tmpl[3])), C.byref(gs) if gates else None)
    assert bpg.lib().bpg_test_template_packed_gated(*args, None, C.c_uint64(0), C.byref(words)) == 0, _err()
    out = np.zeros(max(words.value, 1), np.uint32)
    assert bpg.lib().bpg_test_template_packed_gated(*args, C.c_void_p(out.ctypes.data), C.c_uint64(words.value), C.byref(words)) == 0, _err()
    return out[:words.value]


def oracle_circuit(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def kinds(inst):
    return {int(x) >> 29 for x in inst.term_var}


# ------------------------------------------------------------------------------------------------ 1. the hand-made circuit
@pytest.fixture(scope="module")
def hand():
    """(template made from vector 0, the yardstick assemblies of every vector)"""
    tmpl = template_of(G.hand10(G.HAND_INPUTS[0], G.HAND_VALUES[0], True))
    hosts = [G.hand10(i, v, False).prover.instance() for i, v in zip(G.HAND_INPUTS, G.HAND_VALUES)]
    return tmpl, hosts


def test_hand10_keeps_its_gates_and_resolves_them(hand):
    tmpl, hosts = hand
    inst, prog, hints, values, gates = tmpl
    assert inst.n == G.HAND_N and bpg.VAR_GATED in kinds(inst) and bpg.VAR_INPUT in kinds(inst)
    assert bpg.VAR_GATED in {int(x) >> 29 for x in prog.term_var}
    assert len(gates) >= 10 and all(var.kind <= 3 and p < 4 for var, p in gates)
    hint_rows = [int(prog.lc_ptr[2 * int(m)]) for m in hints.mul]                  # a hint run whose source holds a gate keeps it
    assert any(int(prog.term_var[k]) >> 29 == bpg.VAR_GATED for k in hint_rows)
    for (inputs, vals), host in zip(zip(G.HAND_INPUTS, G.HAND_VALUES), hosts):
        own = G.hand10(inputs, vals, True).prover.instance()                       # the resolved export of the prover that USED gates
        assert kinds(own) <= {0, 1, 2, 3, 4} and kinds(host) <= {0, 1, 2, 3, 4}
        assert witness(own) == witness(host) and meaning_of(own) == meaning_of(host) and own.v == host.v
        assert O.satisfied(oracle_circuit(own), own.v) and O.satisfied(oracle_circuit(host), host.v)


def test_hand10_interpreter_and_slotted_rows(hand):
    tmpl, hosts = hand
    for inputs, host in zip(G.HAND_INPUTS, hosts):
        ins = [sc(x) for x in inputs]
        aL, aR, aO, first = eval_gated(tmpl, host.v, ins)
        assert first is None and (aL, aR, aO) == witness(host), "inputs %r: the interpreter differs from the host assembly with constants" % (inputs,)
        rows = gated_instance(tmpl, ins)
        assert {int(x) >> 29 for x in rows[1]} <= {0, 1, 2, 3, 4}
        assert meaning(*rows) == meaning_of(host), "inputs %r: the resident rows do not mean what the host assembly's rows mean" % (inputs,)
        slotted = O.FlatCircuit(host.n, host.m, host.aL, host.aR, host.aO, *rows)
        assert O.satisfied(slotted, host.v)


def test_hand10_checkpointed_gate(hand):
    """a gate over a checkpointed variable reads the caller's value; a wrong value is reported and not papered over"""
    tmpl, hosts = hand
    host, ins = hosts[3], [sc(x) for x in G.HAND_INPUTS[3]]
    good = host.aO[32 * 3:32 * 4]
    aL, aR, aO, first = eval_gated(tmpl, host.v, ins, [G.HAND_CHECKPOINT], [good])
    assert first is None and (aL, aR, aO) == witness(host)
    bad = sc(int.from_bytes(good, "little") + 1)
    aL2, aR2, aO2, first = eval_gated(tmpl, host.v, ins, [G.HAND_CHECKPOINT], [bad])
    assert first == 0 and aO2[32 * 3:32 * 4] == good and aR2[32 * 4:32 * 5] != aR[32 * 4:32 * 5]      # m4's right list read the caller's value through its gate
    S0, S1 = schedule_gated(tmpl), schedule_gated(tmpl, [G.HAND_CHECKPOINT])
    assert S1["levels"] < S0["levels"]


@pytest.mark.parametrize("K", [3, 65])
def test_hand10_batch(hand, K):
    tmpl, hosts = hand
    ins = [[sc((7 * k + 1) * 2**(3 * k % 250) % L), sc(k % 2), sc(L - 1 - k), sc(2**252 + 9 + k)] for k in range(K)]
    vals = [((k + 2) % L, (L - 5 * k - 1) % L) for k in range(K)]
    vs = [sc(a) + sc(b) for a, b in vals]
    got, firsts = eval_batch_gated(tmpl, vs, ins)
    assert firsts == [None] * K
    for k in (range(K) if K < 10 else (0, 1, 31, 63, 64)):
        aL, aR, aO, _ = eval_gated(tmpl, vs[k], ins[k])
        assert got[k] == (aL, aR, aO), "item %d: the batched interpreter differs from the single one" % k
        host = G.hand10([int.from_bytes(x, "little") for x in ins[k]], vals[k], False).prover.instance()
        assert got[k] == witness(host), "item %d" % k


def test_hand10_stream_and_slots(hand):
    tmpl, hosts = hand
    inst, prog, hints, values, gates = tmpl
    words = packed_gated(tmpl)
    assert 6 in {int(w) >> 29 for w in words}                               # WIT_KIND_INPUT for the constant input terms
    # a pair a constant input term and a gated term share has ONE slot: slots = distinct (input, coefficient index) pairs over both kinds of term
    pairs = set()
    for v, c in zip(inst.term_var, inst.term_coef):
        if int(v) >> 29 == bpg.VAR_INPUT:
            pairs.add((int(v) & 0x1fffffff, int(c)))
        elif int(v) >> 29 == bpg.VAR_GATED:
            pairs.add((gates[int(v) & 0x1fffffff][1], int(c)))
    const_pairs = {(int(v) & 0x1fffffff, int(c)) for v, c in zip(inst.term_var, inst.term_coef) if int(v) >> 29 == bpg.VAR_INPUT}
    gated_pairs = {(gates[int(v) & 0x1fffffff][1], int(c)) for v, c in zip(inst.term_var, inst.term_coef) if int(v) >> 29 == bpg.VAR_GATED}
    assert const_pairs & gated_pairs, "the circuit was to share a pair between a constant and a gated term"
    rp, tv, tc, coef = gated_instance(tmpl, values)
    assert len(coef) // 32 == inst.ncoef + len(pairs) and coef[:32 * inst.ncoef] == inst.coef
    # a gated term whose INPUT is zero is a term of the stream all the same: the stream does not depend on the values
    zero = template_of(G.hand10((0, 0, 0, 0), G.HAND_VALUES[0], True))
    assert (packed_gated(zero) == words).all()


# ------------------------------------------------------------------------------------------------ 2. Merkle paths
@pytest.fixture(scope="module")
def trees():
    """depth -> (levels of the host tree over 2^depth leaves)"""
    return {d: G.host_tree(G.sample_leaves(1 << d, "d%d" % d)) for d in (1, 2, 3)}


@pytest.fixture(scope="module")
def gens():
    return O.Gens(8192)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_path_is_the_reference_circuit_of_every_index(trees, gens, depth):
    lv = trees[depth]
    root = lv[-1][0]
    tmpl = None
    for index in range(1 << depth):
        sib, nodes = G.host_path(lv, index)
        g = G.path_gated(None, index, lv[0][index], sib, root)
        r = G.path_reference(None, index, lv[0][index], sib, root)
        gi, ri = g.prover.instance(), r.prover.instance()
        assert (gi.n, gi.m, gi.q) == (ri.n, ri.m, ri.q) == (1944 * depth, 1, 3888 * depth + 1)
        assert witness(gi) == witness(ri) and gi.v == ri.v, "index %d: witness bytes" % index
        assert kinds(gi) <= {0, 1, 2, 3, 4} and meaning_of(gi) == meaning_of(ri), "index %d: the rows mean something else" % index
        assert g.transcript.state == r.transcript.state
        assert [v for v in G.node_checkpoints(g.prover)] == [v for v in G.node_checkpoints(r.prover)]
        seed = bytes([index + 1]) * 32
        rc1, p1, _ = O.prove(gens, g.transcript.state, oracle_circuit(gi), gi.v_blinding, seed)
        rc2, p2, _ = O.prove(gens, r.transcript.state, oracle_circuit(ri), ri.v_blinding, seed)
        assert rc1 == 0 and rc2 == 0 and p1 == p2, "index %d: the oracle's proofs differ" % index
        # ONE template (made at index 0) under this index's inputs: the interpreter, with and without node checkpoints, and the slotted rows
        if tmpl is None:
            tmpl, cks = template_of(g), G.node_checkpoints(g.prover)
        aL, aR, aO, first = eval_gated(tmpl, ri.v, g.inputs)
        assert first is None and (aL, aR, aO) == witness(ri), "index %d: the template's interpreter" % index
        aL, aR, aO, first = eval_gated(tmpl, ri.v, g.inputs, cks, nodes)
        assert first is None and (aL, aR, aO) == witness(ri), "index %d: the checkpointed interpreter" % index
        if index in (0, (1 << depth) - 1):
            assert meaning(*gated_instance(tmpl, g.inputs)) == meaning_of(ri), "index %d: the resident rows" % index


def test_path_schedule(trees):
    """what the cutting rules give: a node is two segments (one per absorbed block) - the first reads the running hash through its gate, the second the
    first's state and the running hash again.  Without checkpoints the chain is 2 levels per node; with the node hashes checkpointed every node reads the
    caller's value and the whole path is 2 levels."""
    for depth in (1, 2, 3):
        lv = trees[depth]
        sib, nodes = G.host_path(lv, 0)
        g = G.path_gated(None, 0, lv[0][0], sib, lv[-1][0])
        tmpl = template_of(g)
        S = schedule_gated(tmpl)
        assert S["segments"] == 2 * depth and S["seg_first"] == [972 * k for k in range(2 * depth + 1)]
        assert S["seg_level"] == list(range(2 * depth)) and S["levels"] == 2 * depth
        S = schedule_gated(tmpl, G.node_checkpoints(g.prover))
        assert S["seg_first"] == [972 * k for k in range(2 * depth + 1)]
        assert S["seg_level"] == [0, 1] * depth and S["levels"] == 2 and S["level_segments"] == [depth, depth]


def test_path_batch_of_every_index(trees):
    """the four leaves of the depth-2 tree as one batch of the one template, per-item checkpoints; a wrong node fails its item alone"""
    lv = trees[2]
    root = lv[-1][0]
    g0 = G.path_gated(None, 0, lv[0][0], G.host_path(lv, 0)[0], root)
    tmpl, cks = template_of(g0), G.node_checkpoints(g0.prover)
    ins, nodes, hosts = [], [], []
    for index in range(4):
        sib, nd = G.host_path(lv, index)
        ins.append(bpg.merkle_path_inputs(index, sib, root)); nodes.append(nd)
        hosts.append(G.path_reference(None, index, lv[0][index], sib, root).prover.instance())
    got, firsts = eval_batch_gated(tmpl, [h.v for h in hosts], ins, cks, nodes)
    assert firsts == [None] * 4 and got == [witness(h) for h in hosts]
    nodes[2] = [nodes[2][0], sc(7)]
    got, firsts = eval_batch_gated(tmpl, [h.v for h in hosts], ins, cks, nodes)
    assert firsts == [None, None, 1, None] and [got[k] == witness(hosts[k]) for k in range(4)] == [True, True, True, True]


def test_merkle_path_inputs_are_selections():
    sib, root = [sc(11), sc(L - 1), sc(2**252 + 9)], sc(5)
    zero, one = sc(0), sc(1)
    assert bpg.merkle_path_inputs(0b101, sib, root) == [zero, one, sib[0], zero, one, zero, zero, sib[1], zero, one, sib[2], zero, root]
    assert bpg.merkle_path_inputs(0, [], root) == [root]
    with pytest.raises(bpg.BpgError) as e:
        bpg.merkle_path_inputs(8, sib, root)
    assert e.value.status == 4 and "more bits" in str(e.value)


# ------------------------------------------------------------------------------------------------ 3. nothing moves without gates
def test_no_gates_is_the_inputs_path():
    import template_inputs_cases as TC
    from test_template_inputs_host import template_of as template_of_inputs
    cases = [template_of_inputs(hand8(INPUT_VECTORS[1], HAND_VALUES[0], True)), template_of_inputs(TC.build("merkle_wi", 0, True, prover_cls=StubProver)),
             template_of_inputs(TC.build("less_than", 0, True, prover_cls=StubProver))]
    a = workloads.bounds_check_64(None, seed=2, prover_cls=StubProver)
    cases.append((a.prover.instance(),) + tuple(a.prover.witness_program(hints=True)) + ([],))
    for inst, prog, hints, values in cases:
        old = (inst, prog, hints, values)
        for tmpl in ((inst, prog, hints, values, []),):
            assert schedule_gated(tmpl, raw=True) == schedule_inputs(old, len(values), raw=True)
            assert (packed_gated(tmpl) == packed_inputs(old, len(values))).all()
            assert (packed_gated(tmpl, gates=False) == packed_inputs(old, len(values))).all()
    # a prover that made no gate exports an empty table, and its template instance is what it was
    p = hand8(INPUT_VECTORS[1], HAND_VALUES[0], True).prover
    assert p.gates() == []


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_gate_refusals():
    t = bpg.Transcript(b"x"); p = StubProver(None, t)
    _, v0 = p.commit(sc(3), bytes(32))
    x = p.input(sc(2))
    m = p.multiply(LC.of(v0), LC.of(v0))
    g = p.gate(x, m[2])
    assert g.kind == bpg.VAR_GATED and g.index == 0 and p.gate(x, v0).index == 1
    other = StubProver(None, bpg.Transcript(b"y"))
    cases = [((v0, v0), "no public input"), ((bpg.Variable(bpg.VAR_INPUT << 29 | 1), v0), "public input 1 of 1"), ((x, bpg.Variable.One()), "constant One"),
             ((x, x), "a public input"), ((x, g), "gates do not nest"), ((x, bpg.Variable(bpg.VAR_COMMITTED << 29 | 1)), "out of range"),
             ((x, bpg.Variable(bpg.VAR_MULTIPLIER_LEFT << 29 | 1)), "out of range"), ((x, bpg.Variable(7 << 29)), "unknown kind")]
    for args, word in cases:
        with pytest.raises(bpg.BpgError) as e:
            p.gate(*args)
        assert e.value.status == 4 and word in str(e.value), (word, str(e.value))
    with pytest.raises(bpg.BpgError) as e:
        other.gate(x, v0)                                   # an input of another prover: this one has made none
    assert e.value.status == 4 and "public input 0 of 0" in str(e.value)
    assert len(p.gates()) == 2
    # the verifier's side: the same gates in the same order, the same refusals
    v = bpg.Verifier(bpg.Transcript(b"x"))
    c0 = v.commit(bytes(32)); xv = v.input(sc(2))
    with pytest.raises(bpg.BpgError) as e:
        v.gate(xv, bpg.Variable(bpg.VAR_MULTIPLIER_OUTPUT << 29))
    assert e.value.status == 4 and "out of range" in str(e.value)
    assert v.gate(xv, c0) == g and v.gate(xv, c0).index == 1
    for args, word in [((c0, c0), "no public input"), ((xv, xv), "a public input"), ((xv, bpg.Variable.One()), "constant One")]:
        with pytest.raises(bpg.BpgError) as e:
            v.gate(*args)
        assert e.value.status == 4 and word in str(e.value)
    # a term that names a gate nobody made; a buffer takes no gate
    with pytest.raises(bpg.BpgError) as e:
        other.multiply(LC.of(bpg.Variable(bpg.VAR_GATED << 29)), 1)
    assert e.value.status == 4 and "gate" in str(e.value)
    buf = bpg.ConstraintBuffer(p, True)
    with pytest.raises(bpg.BpgError) as e:
        bpg.Equality([LC.of(g)]).prove(buf, [v0], [])
    assert e.value.status == 4 and "buffer" in str(e.value) and "gate" in str(e.value)
    with pytest.raises(bpg.BpgError) as e:                  # the path gadget makes gates: no buffer assembles it
        bpg.MerklePath256(x, v0, [(x, x, x, x)]).prove(buf, [], [])
    assert e.value.status == 4 and "gate" in str(e.value)


def test_kind_6_is_refused_everywhere_else(hand):
    lib = bpg.lib()
    inst, prog, hints, values, gates = hand[0]
    cs, cp, ch, ck, gs, keep = _views(hand[0])
    h = C.c_void_p(7)
    named = lambda: "kind 6" in _err() and "term" in _err() and "gated variable" in _err()
    # the rows name kinds 5 and 6: whichever the check meets first is named; strip the input terms to meet kind 6 alone
    only6 = template_of(only_gates())
    cs6, cp6, ch6, ck6, gs6, keep6 = _views(only6)
    i6 = only6[0]
    assert lib.bpg_r1cs_upload(FAKE, C.byref(cs6), C.byref(h)) == 4 and named() and not h.value
    ts, proof, ln = C.create_string_buffer(203), C.create_string_buffer(4096), C.c_uint64(4096)
    assert lib.bpg_r1cs_prove(FAKE, C.byref(cs6), ts, C.c_uint64(i6.m), i6.v_blinding, bytes(32), C.c_uint32(0), proof, C.byref(ln)) == 4 and named()
    assert proof.raw == bytes(4096) and ts.raw == bytes(203)
    assert lib.bpg_r1cs_verify(FAKE, C.byref(cs6), ts, C.c_uint64(i6.m), bytes(32 * i6.m), bytes(64), C.c_uint64(64), bytes(32), C.c_uint32(0)) == 4 and named()
    arr, states, keep2 = bpg._verify_items([(i6, bytes(203), bytes(32 * i6.m), bytes(64), bytes(32))])
    status = (C.c_int32 * 1)(77)
    assert lib.bpg_r1cs_verify_batch(FAKE, C.c_uint64(1), arr, bytes(32), status) == 4 and named() and status[0] == 77
    barr, bkeep = bpg._batch_items([(i6, bytes(203), i6.v_blinding, bytes(32), 0)])
    assert lib.bpg_r1cs_prove_batch(FAKE, C.c_uint64(1), barr, status) == 4 and named() and status[0] == 4
    one = C.c_uint64(1)
    for call in (lambda: lib.bpg_r1cs_upload_template_checkpointed(FAKE, C.byref(cs6), C.byref(cp6), ch6, C.byref(ck6), C.byref(h)),
                 lambda: lib.bpg_r1cs_upload_template_hinted(FAKE, C.byref(cs6), C.byref(cp6), ch6, C.byref(h)),
                 lambda: lib.bpg_r1cs_upload_template_inputs(FAKE, C.byref(cs6), C.byref(cp6), ch6, C.byref(ck6), one, only6[3][0], C.byref(h)),
                 lambda: lib.bpg_r1cs_upload_template_gated(FAKE, C.byref(cs6), C.byref(cp6), ch6, C.byref(ck6), one, only6[3][0], None, C.byref(h))):
        h = C.c_void_p(7)
        assert call() == 4 and named() and not h.value
    # the rows resolved, the program not: the program's own check names it
    rs = only_gates().prover.instance().cstruct()
    assert lib.bpg_r1cs_upload_template_inputs(FAKE, C.byref(rs), C.byref(cp6), ch6, C.byref(ck6), one, only6[3][0], C.byref(h)) == 4
    assert "kind 6" in _err() and "witness program" in _err() and "gated variable" in _err()


def only_gates():
    """2 multipliers, one input that stands in gates only"""
    t = bpg.Transcript(b"only"); p = StubProver(None, t)
    _, v0 = p.commit(sc(3), bytes(32))
    x = p.input(sc(5))
    m0 = p.multiply(LC.of(p.gate(x, v0)), LC.of(v0))
    p.multiply(LC.of(p.gate(x, m0[2])) * sc(9), LC.of(m0[0]))
    return G.Case(p, t, [], [sc(5)], 2)


def test_upload_refusals_and_served_calls(hand):
    lib = bpg.lib()
    tmpl = hand[0]
    inst, prog, hints, values, gates = tmpl
    cs, cp, ch, ck, gs, keep = _views(tmpl)
    h = C.c_void_p(7)
    iv = b"".join(values)

    def up(table, n_in=4):
        g2, k2 = bpg._gates_cstruct(table)
        return lib.bpg_r1cs_upload_template_gated(FAKE, C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(n_in), iv, C.byref(g2), C.byref(h))
    assert up(gates[:-1]) == 4 and "names gate" in _err() and not h.value                                      # a gate index >= n_gates
    assert up([(bpg.Variable.One(), 0)] + gates[1:]) == 4 and "kind 4" in _err()                               # a gate over One
    assert up([(bpg.Variable(bpg.VAR_COMMITTED << 29 | 2), 0)] + gates[1:]) == 4 and "out of range" in _err()
    assert up([(gates[0][0], 4)] + gates[1:]) == 4 and "public input 4" in _err()
    assert up([(bpg.Variable(bpg.VAR_MULTIPLIER_OUTPUT << 29 | 9), gates[0][1])] + gates[1:]) == 4 and "refers to multiplier 9" in _err()      # a forward reference through a gate
    bad = bpg.WitnessGatesView(3, None, None)
    assert lib.bpg_r1cs_upload_template_gated(FAKE, C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(4), iv, C.byref(bad), C.byref(h)) == 4 and "n_gates without" in _err()
    # a handle without device state, made for a template WITH gates: the calls that serve it get as far as the device, the others refuse it by name
    hd = C.c_void_p()
    assert lib.bpg_test_circuit_handle_gated(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(4), C.byref(gs), C.byref(hd)) == 0, _err()
    try:
        m, zero, first = C.c_uint64(inst.m), C.c_uint64(0), C.c_uint64(5)
        assert lib.bpg_r1cs_assign_inputs(FAKE, hd, m, inst.v, zero, None, zero, None, C.byref(first), C.c_uint64(4), iv) == 4 and "no device state" in _err()
        assert lib.bpg_r1cs_assign(FAKE, hd, m, inst.v, zero, None) == 4 and "bpg_r1cs_assign_inputs" in _err()
        for fn in (lib.bpg_r1cs_template_repeat, lib.bpg_r1cs_template_repeat_inputs):
            out = C.c_void_p(7)
            assert fn(FAKE, hd, C.c_uint64(2), C.byref(out)) == 4 and "gated variables" in _err() and not out.value
        part = (bpg.TemplatePart * 1)(); part[0].tmpl = hd; part[0].count = 2
        for fn in (lib.bpg_r1cs_template_join, lib.bpg_r1cs_template_join_inputs):
            out = C.c_void_p(7)
            assert fn(FAKE, C.c_uint64(1), part, C.byref(out)) == 4 and "gated variables" in _err() and "part 0" in _err() and not out.value
    finally:
        lib.bpg_r1cs_free(None, hd)


def test_symbols_and_header():
    lib = bpg.lib()
    for f in ("bpg_prover_gate", "bpg_verifier_gate", "bpg_prover_gates", "bpg_r1cs_upload_template_gated", "bpg_merkle_path256_new", "bpg_merkle_path_inputs",
              "bpg_test_template_schedule_gated", "bpg_test_template_packed_gated", "bpg_test_template_eval_gated", "bpg_test_template_eval_batch_gated",
              "bpg_test_template_gated_instance", "bpg_test_circuit_handle_gated"):
        assert hasattr(lib, f), f
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "#define BPG_ABI_VERSION 7u" in hdr and "#define BPG_VAR_GATED 6u" in hdr
    assert bpg.VAR_GATED == 6
