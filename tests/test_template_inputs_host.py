"""Public inputs in circuit templates without a GPU (bpg_prover_input, bpg_r1cs_upload_template_inputs, bpg_r1cs_assign_inputs): the host model, the
packer and the interpreter compiled for the host (bpg_test_template_eval_inputs, _eval_batch_inputs: poisoned vectors, the segments of every level in reverse
order), the derived coefficient slots (bpg_test_template_inputs_instance) and every refusal.

The yardstick is never the template: it is a FRESH HOST ASSEMBLY of the same statement with the public values baked in as constants
(template_inputs_cases.py, as_inputs=False), which knows nothing of inputs.  One template is made from one (witness, public values) pair and evaluated under
others."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import checkpoint_cases as CK
import template_inputs_cases as TC
from template_inputs_cases import StubProver, sc, L

FAKE = C.c_void_p(1)            # a context that is never dereferenced: every call below is refused before the device is needed
NONE = 2**64 - 1
LC = bpg.LinearCombination
FIELDS = ("v", "param_values", "transcript_state", "v_blinding", "rng_seed", "flags", "proof_out", "proof_len", "commitments_out", "ck_values", "first_mismatch",
          "input_values")


def _err():
    return (bpg.lib().bpg_last_error() or b"").decode()


def _views(inst, prog, hints, ck_vars=()):
    cs, cp = inst.cstruct(), prog.cstruct()
    ch = hints.cstruct() if hints is not None and len(hints) else None
    ck = bpg._checkpoints_cstruct(list(ck_vars))
    return cs, cp, C.byref(ch) if ch is not None else None, ck, ch


def template_of(case):
    """(instance with its input terms, program, hints, input values) of an assembly made with as_inputs=True"""
    inst, values = case.prover.template_instance()
    prog, hints = case.prover.witness_program(hints=True)
    assert values == case.inputs
    return inst, prog, hints, values


def eval_inputs(tmpl, v, inputs, ck_vars=(), ck_values=None, expect=0):
    inst, prog, hints, _ = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints, ck_vars)
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    first = C.c_uint64(12345)
    st = bpg.lib().bpg_test_template_eval_inputs(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(inputs) if inputs is not None else len(tmpl[3])), v,
                                                 b"".join(ck_values) if ck_values else None, b"".join(inputs) if inputs is not None else None, *out, C.byref(first))
    assert st == expect, _err()
    return out[0].raw, out[1].raw, out[2].raw, None if first.value == NONE else first.value


def eval_batch_inputs(tmpl, vs, inputs):
    inst, prog, hints, _ = tmpl
    K, N = len(vs), 1 << (inst.n - 1).bit_length()
    cs, cp, ch, ck, keep = _views(inst, prog, hints)
    out = [C.create_string_buffer(32 * N * K) for _ in range(3)]
    first = (C.c_uint64 * max(K, 1))(*[12345] * max(K, 1))
    st = bpg.lib().bpg_test_template_eval_batch_inputs(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(len(inputs[0])), C.c_uint64(K), b"".join(vs), None,
                                                       b"".join(b"".join(x) for x in inputs), *out, first)
    assert st == 0, _err()
    assert all(first[k] == NONE for k in range(K))
    res = []
    for k in range(K):
        item = tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out)
        assert all(x[32 * inst.n:] == bytes(32 * (N - inst.n)) for x in item), "item %d: padding rows are not zero" % k
        res.append(tuple(x[:32 * inst.n] for x in item))
    return res


def inputs_instance(tmpl, inputs, params=()):
    """bpg_test_template_inputs_instance -> (row_ptr, term_var, term_coef, coef bytes)"""
    inst, prog, hints, _ = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints)
    rows, terms, coefs = inst.q + 1, inst.nnz + len(prog.param_rows) + 8, inst.ncoef + len(prog.param_rows) + inst.nnz + 8
    rp, tv, tc = np.zeros(rows, np.uint64), np.zeros(terms, np.uint32), np.zeros(terms, np.uint32)
    coef = C.create_string_buffer(32 * coefs)
    nnz, ncoef = C.c_uint64(), C.c_uint64()
    st = bpg.lib().bpg_test_template_inputs_instance(C.byref(cs), C.byref(cp), ch, C.c_uint64(len(inputs)), b"".join(params) or None, b"".join(inputs),
                                                     C.c_void_p(rp.ctypes.data), C.c_uint64(rows), C.c_void_p(tv.ctypes.data), C.c_void_p(tc.ctypes.data), C.c_uint64(terms),
                                                     coef, C.c_uint64(coefs), C.byref(nnz), C.byref(ncoef))
    assert st == 0, _err()
    return rp, tv[:nnz.value], tc[:nnz.value], coef.raw[:32 * ncoef.value]


def meaning(row_ptr, term_var, term_coef, coef):
    """per row: (sum of the constant terms mod l, {variable: summed coefficient mod l, zeros dropped})"""
    cf = [int.from_bytes(coef[32 * i:32 * i + 32], "little") % L for i in range(len(coef) // 32)]
    out = []
    for r in range(len(row_ptr) - 1):
        const, terms = 0, {}
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            var, c = int(term_var[k]), cf[int(term_coef[k])]
            if var >> 29 == bpg.VAR_ONE:
                const = (const + c) % L
            else:
                terms[var] = (terms.get(var, 0) + c) % L
        out.append((const, {v: c for v, c in terms.items() if c}))
    return out


def meaning_of(inst):
    return meaning(inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def witness(inst):
    return inst.aL, inst.aR, inst.aO


# ------------------------------------------------------------------------------------------------ 1. hand-made circuits
INPUT_VECTORS = [(0, L - 1, 2**252 + 9), (5, 7, 13), (L - 1, 2**252 + 1, 0)]
HAND_VALUES = [(3, 4), (2**200 + 1, L - 2), (0, 9)]


def hand8(inputs, values, as_inputs):
    """8 multipliers: an input in a left list (+1), in a right list (-1), in both under general coefficients - the same input under two coefficients and two
    inputs in one row -, in a plain constrain() row, as the whole source of a 4-bit hint run, and once more after it"""
    t = bpg.Transcript(b"hand8"); p = StubProver(None, t)
    pub = TC.Public(p, as_inputs)
    vs = [p.commit(sc(x), bytes(32))[1] for x in values]
    X0, X1, X2 = (pub(sc(x)) for x in inputs)
    m0 = p.multiply(LC.of(vs[0]) + X0, LC.of(vs[1]))
    m1 = p.multiply(LC.of(m0[2]), LC.of(vs[0]) - X1)
    m2 = p.multiply(X0 * sc(5) + LC.of(m1[2]), X0 * sc(L - 3) + X1 + LC.of(vs[1]))
    p.constrain(LC.of(m2[2]) - X2 * sc(7) + X0 + LC.of(9))
    for bit in range(4):
        p.allocate_bit(X2, bit, sc(inputs[2]))
    p.multiply(LC.of(m2[0]) + X2, LC.of(1) + X2 * sc(L - 1))
    return TC.Case(p, t, [], pub.values, 8)


def hand3(inputs, values, as_inputs):
    """3 multipliers, one input: a parameter row beside an input term, and an input that only a constraint names"""
    t = bpg.Transcript(b"hand3"); p = StubProver(None, t)
    pub = TC.Public(p, as_inputs)
    vs = [p.commit(sc(x), bytes(32))[1] for x in values]
    X0, X1, X2 = (pub(sc(x)) for x in inputs)
    m0 = p.multiply(X0, X0)
    m1 = p.multiply(LC.of(m0[2]) + LC.of(vs[0]), X0 * sc(2**130))
    p.multiply(LC.of(m1[0]), LC.of(m1[1]) - X1)
    p.constrain(LC.of(m1[2]) - X2 - X2 + LC.of(4))
    p.mark_param_row(p.num_constraints() - 1)               # its constant 4 is a parameter; the two input terms beside it stay terms of their own
    return TC.Case(p, t, [], pub.values, 4)


@pytest.mark.parametrize("make", [hand8, hand3])
def test_hand_made_circuits(make):
    tmpl = template_of(make(INPUT_VECTORS[1], HAND_VALUES[0], True))
    inst = tmpl[0]
    assert 3 <= inst.n <= 8 and bpg.VAR_INPUT in {int(x) >> 29 for x in inst.term_var}
    for inputs, values in zip(INPUT_VECTORS, HAND_VALUES):
        host = make(inputs, values, False).prover.instance()
        assert bpg.VAR_INPUT not in {int(x) >> 29 for x in host.term_var}
        aL, aR, aO, first = eval_inputs(tmpl, host.v, [sc(x) for x in inputs])
        assert first is None and (aL, aR, aO) == witness(host), "inputs %r: the interpreter differs from the host assembly with constants" % (inputs,)
        got = meaning(*inputs_instance(tmpl, [sc(x) for x in inputs], [sc(4)] * len(tmpl[1].param_rows)))
        assert got == meaning_of(host), "inputs %r: the resident rows do not mean what the host assembly's rows mean" % (inputs,)
        # the resolved export of the prover that USED inputs is that assembly too
        own = make(inputs, values, True).prover.instance()
        assert witness(own) == witness(host) and meaning_of(own) == meaning_of(host) and bpg.VAR_INPUT not in {int(x) >> 29 for x in own.term_var}


def test_hand8_packing_and_schedule():
    tmpl = template_of(hand8(INPUT_VECTORS[1], HAND_VALUES[0], True))
    inst, prog, hints, _ = tmpl
    words = packed_inputs(tmpl, 3)
    kinds = [int(w) >> 29 for w in words]
    assert 6 in kinds and 5 not in kinds                    # WIT_KIND_INPUT in the stream; the instance's kind 5 never reaches it
    S = schedule_inputs(tmpl, 3)
    assert S["levels"] >= 1 and S["seg_level"][0] == 0
    hint_seg = S["seg_first"].index(3)                      # the hint run over one input term: a lane of its own at level 0
    assert S["seg_first"][hint_seg + 1] == 7 and S["seg_level"][hint_seg] == 0
    # one derived slot per distinct (input, coefficient) pair, behind the caller's table
    rp, tv, tc, coef = inputs_instance(tmpl, [sc(x) for x in INPUT_VECTORS[1]])
    pairs = {(int(v) & 0x1fffffff, int(c)) for v, c in zip(inst.term_var, inst.term_coef) if int(v) >> 29 == bpg.VAR_INPUT}
    assert len(coef) // 32 == inst.ncoef + len(pairs) and len(pairs) >= 5
    assert coef[:32 * inst.ncoef] == inst.coef


def schedule_inputs(tmpl, n_in, ck_vars=(), raw=False, expect=0):
    inst, prog, hints, _ = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints, ck_vars)
    buf = C.create_string_buffer(1 << 20)
    st = bpg.lib().bpg_test_template_schedule_inputs(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(n_in), buf, C.c_uint64(len(buf)))
    assert st == expect, _err()
    return buf.value if raw or st else json.loads(buf.value.decode())


def packed_inputs(tmpl, n_in, ck_vars=()):
    inst, prog, hints, _ = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints, ck_vars)
    words = C.c_uint64()
    args = (C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(n_in))
    assert bpg.lib().bpg_test_template_packed_inputs(*args, None, C.c_uint64(0), C.byref(words)) == 0, _err()
    out = np.zeros(max(words.value, 1), np.uint32)
    assert bpg.lib().bpg_test_template_packed_inputs(*args, C.c_void_p(out.ctypes.data), C.c_uint64(words.value), C.byref(words)) == 0, _err()
    return out[:words.value]


# ------------------------------------------------------------------------------------------------ 2. reference gadgets with the public side as inputs
@pytest.fixture(scope="module", params=sorted(TC.GADGETS))
def gadget(request):
    """(name, template of case 0, the host assemblies WITH CONSTANTS of cases 0..2, their input values) - built once per gadget"""
    name = request.param
    tmpl = template_of(TC.build(name, 0, True, prover_cls=StubProver))
    hosts = [TC.build(name, k, False, prover_cls=StubProver).prover.instance() for k in range(3)]
    inputs = [TC.build(name, k, True, prover_cls=StubProver).inputs for k in range(3)]
    return name, tmpl, hosts, inputs


def test_gadget_under_other_public_values(gadget):
    name, tmpl, hosts, inputs = gadget
    assert inputs[1] != inputs[0] or inputs[2] != inputs[0]
    assert len({tuple(x) for x in inputs}) >= 2
    for k in (0, 1, 2):
        aL, aR, aO, first = eval_inputs(tmpl, hosts[k].v, inputs[k])
        assert first is None and (aL, aR, aO) == witness(hosts[k]), "%s case %d: the interpreter differs from the host assembly with constants" % (name, k)
        assert meaning(*inputs_instance(tmpl, inputs[k])) == meaning_of(hosts[k]), "%s case %d: resident rows" % (name, k)


def test_less_than_with_a_public_bound_keeps_its_schedule():
    tmpl = template_of(TC.build("less_than", 0, True, prover_cls=StubProver))
    S = schedule_inputs(tmpl, 1)
    assert S["segments"] == 4 and S["levels"] == 1 and S["seg_first"] == [0, 126, 252, 378, 379]
    const = TC.build("less_than", 0, False, prover_cls=StubProver).prover
    prog, hints = const.witness_program(hints=True)
    S0 = schedule_inputs((const.instance(), prog, hints, []), 0)
    assert (S0["segments"], S0["levels"]) == (4, 1)


def test_merkle_with_checkpoints_and_inputs():
    """the (W I) node with its digest checkpointed: the caller's digest is read, and a wrong one is reported - inputs and checkpoints side by side"""
    a = TC.build("merkle_wi", 1, True, prover_cls=StubProver)
    tmpl = template_of(a)
    notes = a.prover.noted()
    ck_vars = [v for v, _, last in notes if last]
    assert len(ck_vars) == 1
    host = TC.build("merkle_wi", 2, False, prover_cls=StubProver)
    hi = host.prover.instance()
    inputs = TC.build("merkle_wi", 2, True, prover_cls=StubProver).inputs
    aL, aR, aO, first = eval_inputs(tmpl, hi.v, inputs, ck_vars, [host.root])
    assert first is None and (aL, aR, aO) == witness(hi)
    aL, aR, aO, first = eval_inputs(tmpl, hi.v, inputs, ck_vars, [sc(5)])
    assert first == 0


# ------------------------------------------------------------------------------------------------ 3. the batch hook
@pytest.mark.parametrize("K", [3, 65])
def test_batch_every_item_its_own_inputs(K):
    tmpl = template_of(hand8(INPUT_VECTORS[1], HAND_VALUES[0], True))
    ins = [[sc((7 * k + 1) * 2**(3 * k % 250) % L), sc(L - 1 - k), sc(2**252 + k)] for k in range(K)]
    vs = [sc(k + 2) + sc(L - 5 * k - 1) for k in range(K)]
    assert len({tuple(x) for x in ins}) == K
    got = eval_batch_inputs(tmpl, vs, ins)
    for k in (range(K) if K < 10 else (0, 1, 31, 63, 64)):
        aL, aR, aO, _ = eval_inputs(tmpl, vs[k], ins[k])
        assert got[k] == (aL, aR, aO), "item %d: the batched interpreter differs from the single one" % k
    # and the single one is the host assembly (item 64: one past a 64-lane block)
    k = K - 1
    host = hand8([int.from_bytes(x, "little") for x in ins[k]], [int.from_bytes(vs[k][:32], "little"), int.from_bytes(vs[k][32:], "little")], False).prover.instance()
    assert got[k] == witness(host)


def test_batch_less_than_three_bounds():
    name = "less_than"
    tmpl = template_of(TC.build(name, 0, True, prover_cls=StubProver))
    hosts = [TC.build(name, k, False, prover_cls=StubProver).prover.instance() for k in range(3)]
    inputs = [TC.build(name, k, True, prover_cls=StubProver).inputs for k in range(3)]
    assert eval_batch_inputs(tmpl, [h.v for h in hosts], inputs) == [witness(h) for h in hosts]


# ------------------------------------------------------------------------------------------------ 4. nothing moves without inputs
def test_no_inputs_is_the_checkpointed_path():
    from test_template_checkpoints_host import schedule_ck, packed
    cases = [(workloads.less_than_126(None, seed=1, prover_cls=StubProver), []), (workloads.bounds_check_64(None, seed=2, prover_cls=StubProver), [])]
    p = CK.path(None, 1, depth=2, seed=1, prover_cls=StubProver)
    cases.append((p, p.ck_vars))
    for a, ck_vars in cases:
        inst = a.prover.instance()
        prog, hints = a.prover.witness_program(hints=True)
        tmpl = (inst, prog, hints, [])
        assert schedule_inputs(tmpl, 0, ck_vars, raw=True) == schedule_ck(inst, prog, hints, ck_vars, raw=True)
        assert (packed_inputs(tmpl, 0, ck_vars) == packed(inst, prog, hints, ck_vars)).all()
        # a prover that made no input exports the same instance both ways
        ti, values = a.prover.template_instance()
        assert values == [] and (ti.coef, ti.aL, ti.aR, ti.aO) == (inst.coef, inst.aL, inst.aR, inst.aO)
        assert (ti.row_ptr == inst.row_ptr).all() and (ti.term_var == inst.term_var).all() and (ti.term_coef == inst.term_coef).all()


def test_resolved_export_never_shows_an_input():
    for name in sorted(TC.GADGETS):
        a = TC.build(name, 1, True, prover_cls=StubProver)
        b = TC.build(name, 1, False, prover_cls=StubProver)
        ia, ib = a.prover.instance(), b.prover.instance()
        assert bpg.VAR_INPUT not in {int(x) >> 29 for x in ia.term_var}
        assert witness(ia) == witness(ib) and meaning_of(ia) == meaning_of(ib) and ia.v == ib.v
        assert a.transcript.state == b.transcript.state         # an input adds no transcript byte
    v = bpg.Verifier(bpg.Transcript(b"LessThan"))
    TC.build("less_than", 1, False, prover_cls=StubProver).replay(v, as_inputs_=True)
    w = bpg.Verifier(bpg.Transcript(b"LessThan"))
    TC.build("less_than", 1, False, prover_cls=StubProver).replay(w)
    assert bpg.VAR_INPUT not in {int(x) >> 29 for x in v.instance().term_var} and meaning_of(v.instance()) == meaning_of(w.instance())


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_kind_5_is_refused_everywhere_else():
    lib = bpg.lib()
    tmpl = template_of(hand8(INPUT_VECTORS[1], HAND_VALUES[0], True))
    inst, prog, hints, values = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints)
    h = C.c_void_p(7)
    named = lambda: "kind 5" in _err() and "term" in _err() and "public input" in _err()
    assert lib.bpg_r1cs_upload(FAKE, C.byref(cs), C.byref(h)) == 4 and named() and not h.value
    ts, proof, ln = C.create_string_buffer(203), C.create_string_buffer(4096), C.c_uint64(4096)
    assert lib.bpg_r1cs_prove(FAKE, C.byref(cs), ts, C.c_uint64(inst.m), inst.v_blinding, bytes(32), C.c_uint32(0), proof, C.byref(ln)) == 4 and named()
    assert proof.raw == bytes(4096) and ts.raw == bytes(203)
    assert lib.bpg_r1cs_verify(FAKE, C.byref(cs), ts, C.c_uint64(inst.m), bytes(32 * inst.m), bytes(64), C.c_uint64(64), bytes(32), C.c_uint32(0)) == 4 and named()
    # the batch calls: verify_batch refuses the call, prove_batch the item - both before the context is looked at
    arr, states, keep2 = bpg._verify_items([(inst, bytes(203), bytes(32 * inst.m), bytes(64), bytes(32))])
    status = (C.c_int32 * 1)(77)
    assert lib.bpg_r1cs_verify_batch(FAKE, C.c_uint64(1), arr, bytes(32), status) == 4 and named() and status[0] == 77
    barr, bkeep = bpg._batch_items([(inst, bytes(203), inst.v_blinding, bytes(32), 0)])
    assert lib.bpg_r1cs_prove_batch(FAKE, C.c_uint64(1), barr, status) == 4 and named() and status[0] == 4
    # the older template uploads: the rows, and a program alone
    for call in (lambda: lib.bpg_r1cs_upload_template_checkpointed(FAKE, C.byref(cs), C.byref(cp), ch, C.byref(ck), C.byref(h)),
                 lambda: lib.bpg_r1cs_upload_template_hinted(FAKE, C.byref(cs), C.byref(cp), ch, C.byref(h))):
        h = C.c_void_p(7)
        assert call() == 4 and named() and not h.value
    resolved = hand8(INPUT_VECTORS[1], HAND_VALUES[0], True).prover.instance()
    rs = resolved.cstruct()
    assert lib.bpg_r1cs_upload_template_checkpointed(FAKE, C.byref(rs), C.byref(cp), ch, C.byref(ck), C.byref(h)) == 4 and "kind 5" in _err() and "witness program" in _err()
    with pytest.raises(bpg.BpgError) as e:                  # a linear combination with an input of another prover
        bpg.Prover(None, bpg.Transcript(b"x")).multiply(bpg.Variable(bpg.VAR_INPUT << 29), 1)
    assert e.value.status == 4 and "public input" in str(e.value)


def test_upload_and_assign_refusals():
    lib = bpg.lib()
    tmpl = template_of(hand8(INPUT_VECTORS[1], HAND_VALUES[0], True))
    inst, prog, hints, values = tmpl
    cs, cp, ch, ck, keep = _views(inst, prog, hints)
    h = C.c_void_p(7)
    up = lambda n_in, vals: lib.bpg_r1cs_upload_template_inputs(FAKE, C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(n_in), vals, C.byref(h))
    assert up(2, b"".join(values[:2])) == 4 and "public input 2" in _err() and "takes 2" in _err() and not h.value       # an input index >= n_inputs
    assert up(3, None) == 4 and "carries a witness" in _err()                                                              # NULL values with n_inputs > 0
    schedule_inputs(tmpl, 2, expect=4)
    assert "public input 2" in _err()
    eval_inputs(tmpl, inst.v, None, expect=4)
    assert "input_values is null" in _err()
    # an input term in a hint's right list: the first hinted multiplier's source moved to the right
    lc = prog.lc_ptr.copy(); lc[7] = lc[6]
    bad = bpg.WitnessProgram(lc, prog.term_var, prog.term_coef)
    schedule_inputs((inst, bad, hints, values), 3, expect=4)
    assert "right list that names a public input" in _err()
    # a handle without device state, made for a template WITH inputs
    hd = C.c_void_p()
    assert lib.bpg_test_circuit_handle_inputs(C.byref(cs), C.byref(cp), ch, C.byref(ck), C.c_uint64(3), C.byref(hd)) == 0, _err()
    try:
        m, iv = C.c_uint64(inst.m), b"".join(values)
        zero, first = C.c_uint64(0), C.c_uint64(5)
        assert lib.bpg_r1cs_assign(FAKE, hd, m, inst.v, zero, None) == 4 and "public inputs" in _err() and "bpg_r1cs_assign_inputs" in _err()
        assert lib.bpg_r1cs_assign_checkpointed(FAKE, hd, m, inst.v, zero, None, zero, None, C.byref(first)) == 4 and "public inputs" in _err()
        assert lib.bpg_r1cs_assign_inputs(FAKE, hd, m, inst.v, zero, None, zero, None, C.byref(first), C.c_uint64(3), None) == 4 and "input_values is null" in _err()
        assert lib.bpg_r1cs_assign_inputs(FAKE, hd, m, inst.v, zero, None, zero, None, C.byref(first), C.c_uint64(2), iv) == 4 and "n_inputs does not match" in _err()
        assert lib.bpg_r1cs_assign_inputs(FAKE, hd, m, inst.v, zero, None, zero, None, C.byref(first), C.c_uint64(3), iv) == 4 and "no device state" in _err()
        # the older batch calls: refused whole, nothing written
        res = bpg.ResidentCircuit(None, None, inst.n, inst.m, n_params=0)
        state = bytes(203)
        item = (inst.v, [], state, inst.v_blinding, bytes(32), 0)
        two = C.c_uint64(2)
        for struct, call in ((bpg._TemplateItem, lambda a, s: lib.bpg_r1cs_prove_template_batch(FAKE, hd, two, a, s)),
                             (bpg._TemplateCommitItem, lambda a, s: lib.bpg_r1cs_prove_template_batch_commit(FAKE, hd, two, a, s)),
                             (bpg._TemplateCkItem, lambda a, s: lib.bpg_r1cs_prove_template_batch_checkpointed(FAKE, hd, two, a, C.c_int32(0), s))):
            arr, keep2 = res._template_items([item] * 2, struct)
            status = (C.c_int32 * 2)(77, 77)
            assert call(arr, status) == 4 and "public inputs" in _err() and "bpg_r1cs_prove_template_batch_inputs" in _err()
            assert list(status) == [77, 77] and all(k[1].raw == bytes(len(k[1])) and k[0].raw[:203] == state for k in keep2)
        arr, keep2 = res._template_items([item] * 2, bpg._TemplateInItem)
        status = (C.c_int32 * 2)(77, 77)
        assert lib.bpg_r1cs_prove_template_batch_inputs(FAKE, hd, two, arr, C.c_int32(0), status) == 4 and "no device state" in _err() and list(status) == [77, 77]
        # repeat and join
        out = C.c_void_p(7)
        assert lib.bpg_r1cs_template_repeat(FAKE, hd, C.c_uint64(2), C.byref(out)) == 4 and "public inputs" in _err() and not out.value
        part = (bpg.TemplatePart * 1)(); part[0].tmpl = hd; part[0].count = 2
        out = C.c_void_p(7)
        assert lib.bpg_r1cs_template_join(FAKE, C.c_uint64(1), part, C.byref(out)) == 4 and "public inputs" in _err() and "part 0" in _err() and not out.value
    finally:
        lib.bpg_r1cs_free(None, hd)


def test_symbols_header_and_item_layout(tmp_path):
    lib = bpg.lib()
    for f in ("bpg_prover_input", "bpg_verifier_input", "bpg_prover_template_instance", "bpg_r1cs_upload_template_inputs", "bpg_r1cs_assign_inputs",
              "bpg_r1cs_prove_template_batch_inputs", "bpg_test_template_schedule_inputs", "bpg_test_template_eval_inputs", "bpg_test_template_eval_batch_inputs",
              "bpg_test_template_inputs_instance"):
        assert hasattr(lib, f), f
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "bpg_template_in_item" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)
    assert re.search(r"#define BPG_ABI_VERSION 7u", hdr) and re.search(r"#define BPG_VAR_INPUT 5u", hdr)
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_template_in_item, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%zu' + " %zu" * len(FIELDS) +
                   '\\n", sizeof(bpg_template_in_item), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert [f for f, _ in bpg._TemplateInItem._fields_] == list(FIELDS)
    assert [f for f, _ in bpg._TemplateCkItem._fields_] == list(FIELDS[:11])
    assert [C.sizeof(bpg._TemplateInItem)] + [getattr(bpg._TemplateInItem, f).offset for f in FIELDS] == want
