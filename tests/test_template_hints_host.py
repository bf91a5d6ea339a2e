"""Range-proof circuits as templates, without a GPU: the bit hints a prover records, their schedule, the device's interpreter compiled for the host, and
the refusals of the hinted calls.

Two yardsticks, both independent of the code under test: the EXISTING host assembly (a_L, a_R, a_O as the prover exported them, for the witness the
template is evaluated on), and `evaluate` below - Python integers mod l read straight off the program and the hints.  Where a committed value is not
canonical the two differ by design (include/bpg.h: the device takes bits of the value mod l, range_proof reads raw bytes); the test of that case asserts
the documented side only.

Schedule numbers derived by hand: a range proof names its source and nothing else, so the bits of one source are one segment; over a committed value
that segment sits at level 0.  BoundsCheck (two ranges over two derived values): 2 segments, 1 level.  LessThan: three ranges (left, right, delta) and the
product delta * delta^-1, which names a committed value no earlier multiplier named: 4 segments, 1 level, n = 3 * 126 + 1.  A two-leaf Merkle node (two
absorbed blocks: segments at levels 0 and 1) followed by a range over the node's hash: a third segment at level 2."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
from test_template_host import StubProver, schedule, check_invariant, _err, _ints

L = bpg.L
ONE = (1).to_bytes(32, "little")
sc = lambda x: x.to_bytes(32, "little")
EDGE_VALUES = [0, 2**64 - 1, 2**64 + 5, (1 << 200) | (1 << 63) | 3, L - 1]


def schedule_hinted(inst, prog, hints):
    cs, cp, ch = inst.cstruct(), prog.cstruct(), hints.cstruct()
    buf = C.create_string_buffer(1 << 20)
    assert bpg.lib().bpg_test_template_schedule_hinted(C.byref(cs), C.byref(cp), C.byref(ch), buf, C.c_uint64(len(buf))) == 0, _err()
    return json.loads(buf.value.decode())


def evaluate(inst, prog, hints, v):
    """the program and its hints read independently: Python integers mod l, from the committed values alone"""
    coef, v = _ints(inst.coef), [x % L for x in _ints(v)]
    vals = ([], [], [], v)
    hint = {int(m): (int(k), int(a)) for m, k, a in zip(hints.mul, hints.kind, hints.arg)}
    for i in range(inst.n):
        lr = []
        for a, b in ((prog.lc_ptr[2 * i], prog.lc_ptr[2 * i + 1]), (prog.lc_ptr[2 * i + 1], prog.lc_ptr[2 * i + 2])):
            acc = 0
            for k in range(int(a), int(b)):
                kind, idx = int(prog.term_var[k]) >> 29, int(prog.term_var[k]) & 0x1fffffff
                assert kind == 4 or kind == 3 or idx < i
                acc += coef[prog.term_coef[k]] * (1 if kind == 4 else vals[kind][idx])
            lr.append(acc % L)
        if i in hint:
            assert hint[i][0] == bpg.HINT_BIT_PAIR and prog.lc_ptr[2 * i + 1] == prog.lc_ptr[2 * i + 2]
            b = (lr[0] >> hint[i][1]) & 1
            lr = [1 - b, b]
        vals[0].append(lr[0]); vals[1].append(lr[1]); vals[2].append(lr[0] * lr[1] % L)
    return tuple(b"".join(sc(x) for x in vals[k]) for k in range(3))


def eval_host(inst, prog, hints, v):
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    cs, cp, ch = inst.cstruct(), prog.cstruct(), hints.cstruct()
    assert bpg.lib().bpg_test_template_eval_hinted(C.byref(cs), C.byref(cp), C.byref(ch), v, *out) == 0, _err()
    return tuple(o.raw for o in out)


def eval_batch_host(inst, prog, hints, vs):
    """-> per item (a_L, a_R, a_O) of n rows each, after checking that rows [n, N) of every item are zero"""
    N = 1
    while N < inst.n:
        N *= 2
    out = [C.create_string_buffer(32 * N * len(vs)) for _ in range(3)]
    cs, cp, ch = inst.cstruct(), prog.cstruct(), hints.cstruct()
    assert bpg.lib().bpg_test_template_eval_batch_hinted(C.byref(cs), C.byref(cp), C.byref(ch), C.c_uint64(len(vs)), b"".join(vs), *out) == 0, _err()
    res = []
    for k in range(len(vs)):
        item = tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out)
        assert all(x[32 * inst.n:] == bytes(32 * (N - inst.n)) for x in item), "item %d: padding rows are not zero" % k
        res.append(tuple(x[:32 * inst.n] for x in item))
    return res


def exported(p):
    inst = p.instance()
    prog, hints = p.witness_program(hints=True)
    return inst, prog, hints


def bounds_host(values):
    """BoundsCheck over [0, 2^64) assembled by the host for ANY three committed values (witness, a, b): the derived values need not come from preprocess"""
    p = StubProver(None, bpg.Transcript(b"BoundsCheck"))
    vs = [p.commit(v, bytes(32))[1] for v in values]
    bpg.BoundsCheck(bytes(8), b"\xff" * 8).prove(p, vs[:1], [(values[1], vs[1]), (values[2], vs[2])])
    return p


def check_against_host(template, provers):
    """the template of one witness, evaluated on the committed values of others, singly and batched, against their host assemblies and `evaluate`"""
    inst, prog, hints = template
    insts = [q.instance() for q in provers]
    for k, other in enumerate(insts):
        want = (other.aL, other.aR, other.aO)
        assert evaluate(inst, prog, hints, other.v) == want, "witness %d: the independent reading differs from the host assembly" % k
        assert eval_host(inst, prog, hints, other.v) == want, "witness %d: the interpreter differs from the host assembly" % k
    got = eval_batch_host(inst, prog, hints, [o.v for o in insts])
    assert got == [(o.aL, o.aR, o.aO) for o in insts], "the batched interpreter differs from the single one"


def test_bounds_check_records_its_hints():
    p = workloads.bounds_check_64(None, seed=1, prover_cls=StubProver).prover
    inst, prog, hints = exported(p)
    assert inst.n == 128 and len(hints) == 128
    assert list(hints.mul) == list(range(128)) and set(hints.kind) == {bpg.HINT_BIT_PAIR} and list(hints.arg) == list(range(64)) * 2
    assert len(prog.lc_ptr) == 257 and len(prog.term_var) == 128
    for i in range(128):                                     # the source of bit i: the derived committed variable a (1) resp. b (2), coefficient one
        assert prog.lc_ptr[2 * i] == i and prog.lc_ptr[2 * i + 1] == prog.lc_ptr[2 * i + 2] == i + 1
        assert prog.term_var[i] == (3 << 29 | (1 + i // 64))
        assert inst.coef[32 * int(prog.term_coef[i]):32 * int(prog.term_coef[i]) + 32] == ONE
    S = schedule_hinted(inst, prog, hints)
    check_invariant(inst, prog, S)
    assert S["segments"] == 2 and S["levels"] == 1 and S["seg_first"] == [0, 64, 128] and S["seg_level"] == [0, 0]
    with pytest.raises(bpg.BpgError) as e:                   # the plain export still refuses the circuit
        p.witness_program()
    assert e.value.status == 4 and "free multiplier" in str(e.value)


def test_recording_leaves_the_instance_alone():
    """the hints enter the coefficient dictionary only at export: the instance exported after a hinted export equals the one exported before, and that of a
    prover that was never asked for hints"""
    a = workloads.bounds_check_64(None, seed=3, prover_cls=StubProver).prover
    b = workloads.bounds_check_64(None, seed=3, prover_cls=StubProver).prover
    before = a.instance()
    a.witness_program(hints=True)
    for x in (a.instance(), b.instance()):
        assert (x.n, x.q, x.ncoef, x.coef, x.aL, x.aR, x.aO) == (before.n, before.q, before.ncoef, before.coef, before.aL, before.aR, before.aO)
        assert (x.row_ptr == before.row_ptr).all() and (x.term_var == before.term_var).all() and (x.term_coef == before.term_coef).all()


def test_bounds_check_evaluation():
    template = exported(workloads.bounds_check_64(None, seed=1, prover_cls=StubProver).prover)
    others = [workloads.bounds_check_64(None, seed=s, prover_cls=StubProver).prover for s in (2, 3, 4, 5)]
    assert len({o.instance().v for o in others}) == 4
    edges = [bounds_host([sc(7), sc(x), sc(y)]) for x, y in zip(EDGE_VALUES, reversed(EDGE_VALUES))]
    check_against_host(template, others + edges)
    # and the bits themselves, for one edge value: l - 1 in the first range
    inst = edges[-1].instance()
    assert [int.from_bytes(inst.aR[32 * i:32 * i + 32], "little") for i in range(64)] == [((L - 1) >> i) & 1 for i in range(64)]


def test_less_than_workload():
    a = workloads.less_than_126(None, seed=1, prover_cls=StubProver)
    template = exported(a.prover)
    inst, prog, hints = template
    assert inst.n == 3 * 126 + 1 and inst.m == 4 and len(hints) == 378 and list(hints.arg) == list(range(126)) * 3
    S = schedule_hinted(inst, prog, hints)
    check_invariant(inst, prog, S)
    assert S["seg_first"] == [0, 126, 252, 378, 379] and S["levels"] == 1
    others = [workloads.less_than_126(None, seed=s, prover_cls=StubProver).prover for s in (2, 3, 4)]
    check_against_host(template, [a.prover] + others)


def mixed(leaf_ints):
    """a two-leaf MerkleTree256 and a 64-bit range proof over the node's hash (the output of the last MiMC multiplier)"""
    p = StubProver(None, bpg.Transcript(b"mixed"))
    vs = [p.commit(sc(x), bytes(32))[1] for x in leaf_ints]
    bpg.MerkleTree256(bytes(32), [], bpg.vars_to_lc(vs), "(W W)").prove(p, [], [])
    n0 = p.get_num_multiplications()
    assert n0 == 1944
    bpg.range_proof(p, bpg.Variable(2 << 29 | (n0 - 1)), 64, p.instance().aO[-32:])
    return p


def test_mixed_circuit():
    template = exported(mixed([11, 12]))
    inst, prog, hints = template
    assert inst.n == 1944 + 64 and list(hints.mul) == list(range(1944, 2008))
    S = schedule_hinted(inst, prog, hints)
    check_invariant(inst, prog, S)
    assert S["seg_first"] == [0, 972, 1944, 2008] and S["seg_level"] == [0, 1, 2]      # the hinted segment one level above the segment it reads
    check_against_host(template, [mixed([11, 12]), mixed([2**200 + 1, 5]), mixed([L - 1, 0])])


def test_allocate_bit_directly():
    """a host that drives the mirror itself: bits of 3 * v0 + 5, a source whose coefficient 3 appears in no constraint (it enters the table at export)"""
    def build(x):
        p = StubProver(None, bpg.Transcript(b"direct"))
        v = p.commit(sc(x), bytes(32))[1]
        src = bpg.LinearCombination.of(v) * sc(3) + 5
        val = sc((3 * x + 5) % L)
        for bit in (0, 7, 200, 255):
            l, r, o = p.allocate_bit(src, bit, val)
            p.constrain(bpg.LinearCombination.of(o))
        return p
    template = exported(build(9))
    inst, prog, hints = template
    assert inst.n == 4 and list(hints.arg) == [0, 7, 200, 255] and sc(3) in [inst.coef[i:i + 32] for i in range(0, len(inst.coef), 32)]
    assert schedule_hinted(inst, prog, hints)["segments"] == 1
    check_against_host(template, [build(9), build(2**250 + 77), build(L - 2)])
    with pytest.raises(bpg.BpgError) as e:
        StubProver(None, bpg.Transcript(b"direct")).allocate_bit(bpg.Variable.One(), 256, bytes(32))
    assert e.value.status == 4


def test_a_committed_source_above_l_takes_the_bits_of_the_value_mod_l():
    """the documented semantics (include/bpg.h), asserted on their own: NOT compared with the host's raw-byte bits, which differ here"""
    raw = (L + 5) | (1 << 254)
    assert L <= raw < 2**255
    p = StubProver(None, bpg.Transcript(b"unreduced"))
    v = p.commit(sc(raw), bytes(32))[1]
    bpg.range_proof(p, v, 64, sc(raw))
    inst, prog, hints = exported(p)
    aL, aR, aO = eval_host(inst, prog, hints, sc(raw))
    bits = [((raw % L) >> i) & 1 for i in range(64)]
    assert _ints(aR) == bits and _ints(aL) == [1 - b for b in bits] and aO == bytes(32 * 64)
    assert eval_batch_host(inst, prog, hints, [sc(raw), sc(raw % L)]) == [(aL, aR, aO)] * 2


def test_free_multipliers_stay_refused():
    p = workloads.bounds_check_64(None, seed=1, prover_cls=StubProver).prover
    p.allocate_multiplier((ONE, bytes(32)))
    with pytest.raises(bpg.BpgError) as e:
        p.witness_program(hints=True)
    assert e.value.status == 4 and "multiplier 128 is a free multiplier" in str(e.value)
    q = StubProver(None, bpg.Transcript(b"alloc"))
    q.allocate(ONE); q.allocate(ONE)
    with pytest.raises(bpg.BpgError) as e:
        q.witness_program(hints=True)
    assert e.value.status == 4 and "free multiplier" in str(e.value)


def test_hinted_upload_refusals_need_no_device():
    lib = bpg.lib()
    inst, prog, hints = exported(workloads.bounds_check_64(None, seed=1, prover_cls=StubProver).prover)
    cs, cp = inst.cstruct(), prog.cstruct()

    def refused(word, prog_c=None, mul=hints.mul, kind=hints.kind, arg=hints.arg, view=None):
        ch = view if view is not None else bpg.WitnessHints(mul, kind, arg).cstruct()
        h = C.c_void_p(7)
        rc = lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(prog_c or cp), C.byref(ch), C.byref(h))
        assert rc == 4 and not h.value and word in _err(), (rc, _err())
        h = C.c_void_p(7)                                    # the upload itself, with a context that is never dereferenced
        assert lib.bpg_r1cs_upload_template_hinted(C.c_void_p(1), C.byref(cs), C.byref(prog_c or cp), C.byref(ch), C.byref(h)) == 4 and not h.value

    null = bpg.WitnessHintsView(); null.n_hints = 5
    refused("hint arrays", view=null)
    m = hints.mul.copy(); m[-1] = inst.n
    refused("out of range", mul=m)
    m = hints.mul.copy(); m[1] = m[0]
    refused("ascending", mul=m)
    m = hints.mul.copy(); m[4], m[5] = m[5], m[4]
    refused("ascending", mul=m)
    k = hints.kind.copy(); k[3] = 2
    refused("unknown hint kind", kind=k)
    a = hints.arg.copy(); a[3] = 256
    refused("256 bits", arg=a)
    ptr = prog.lc_ptr.copy(); ptr[1] = 0                     # multiplier 0: the term moves from the left list to the right list
    refused("right list", prog_c=bpg.WitnessProgram(ptr, prog.term_var, prog.term_coef).cstruct())
    tv = prog.term_var.copy(); tv[5] = 1 << 29 | 5           # the source of multiplier 5 names multiplier 5
    refused("earlier", prog_c=bpg.WitnessProgram(prog.lc_ptr, tv, prog.term_coef).cstruct())
    tv = prog.term_var.copy(); tv[5] = 2 << 29 | 127
    refused("earlier", prog_c=bpg.WitnessProgram(prog.lc_ptr, tv, prog.term_coef).cstruct())
    # without hints (NULL or n_hints = 0) the hinted calls are the plain ones: this program, all of whose right lists are empty, is then a circuit of products by zero
    h = C.c_void_p()
    none = bpg.WitnessHintsView()
    for ch in (None, C.byref(none)):
        assert lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(cp), ch, C.byref(h)) == 0 and h.value, _err()
        lib.bpg_r1cs_free(None, h)
    # a handle made with hints is a template like any other
    ch = hints.cstruct()
    assert lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(cp), C.byref(ch), C.byref(h)) == 0, _err()
    try:
        assert lib.bpg_r1cs_assign(C.c_void_p(1), h, C.c_uint64(2), bytes(64), C.c_uint64(0), None) == 4 and "m does not match" in _err()
        assert lib.bpg_r1cs_assign(C.c_void_p(1), h, C.c_uint64(3), bytes(96), C.c_uint64(0), None) == 4 and "no device state" in _err()
    finally:
        lib.bpg_r1cs_free(None, h)


def test_plain_programs_schedule_as_before():
    """hints == NULL: the hinted hook is the plain one"""
    a = workloads.mimc_preimage(None, nbytes=40, seed=2, prover_cls=StubProver)
    inst = a.prover.instance()
    prog, hints = a.prover.witness_program(hints=True)
    assert len(hints) == 0
    assert schedule_hinted(inst, prog, hints) == schedule(inst, a.prover.witness_program())


def test_template_without_a_context_is_refused():
    with pytest.raises(bpg.BpgError) as e:
        workloads.bounds_check_64(None, seed=1, prover_cls=StubProver).prover.template(None)
    assert e.value.status == 4


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [a.strip() for a in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    hints = "const bpg_witness_hints *hints"
    assert proto("bpg_r1cs_upload_template_hinted") == ["bpg_ctx *ctx", "const bpg_r1cs_instance *inst", "const bpg_witness_program *program", hints, "bpg_circuit **out"]
    assert proto("bpg_prover_witness_program_hinted") == ["bpg_prover *p", "bpg_witness_program *program_out", "bpg_witness_hints *hints_out"]
    assert proto("bpg_prover_allocate_bit") == ["bpg_prover *p", "const bpg_lc *source", "uint32_t bit", "const uint8_t source_value[32]", "uint32_t vars_out[3]"]
    for name in ("schedule", "eval", "eval_batch"):
        assert proto("bpg_test_template_%s_hinted" % name)[:3] == ["const bpg_r1cs_instance *inst", "const bpg_witness_program *program", hints]
    assert proto("bpg_test_circuit_handle_hinted") == ["const bpg_r1cs_instance *inst", "const bpg_witness_program *program", hints, "bpg_circuit **out"]
    assert [f for f, _ in bpg.WitnessHintsView._fields_] == ["n_hints", "hint_mul", "hint_kind", "hint_arg"]
    assert [f for f, _ in bpg.WitnessProgramView._fields_] == ["lc_ptr", "term_var", "term_coef", "n_params", "param_rows"]     # frozen: untouched
    assert "bpg_witness_hints" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)
    assert re.search(r"#define BPG_HINT_BIT_PAIR 1u", hdr) and bpg.HINT_BIT_PAIR == 1
