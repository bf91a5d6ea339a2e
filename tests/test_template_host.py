"""Circuit templates without a GPU: the witness program a prover records, its schedule, and the refusals of the template calls.

The yardstick is the EXISTING host assembly: a program is right when an independent reading of it - Python integers mod l, from the committed values
alone - gives the a_L, a_R, a_O the prover itself exported.  That recording changes nothing the prover exported before (instance bytes, transcript state
of every tests/golden/assembly.json circuit) is what tests/test_assembly_fixtures.py shows by passing unmodified; it is not repeated here.

Schedule numbers derived by hand (a MiMC sponge absorbs a block in 486 rounds of two multipliers, `t * t` and `t^2 * t`: 972 multipliers; within a block
every round reads the previous round's output and the block, nothing else, so one block is one segment):
  * full tree of 8 leaves: 4 + 2 + 1 = 7 nodes, each node's sponge absorbs its two children -> 14 segments, n = 14 * 972 = 13,608.  A node over two leaves:
    first block level 0 (it reads a committed leaf only), second block level 1 (it reads the first block's state).  A node of height 2 absorbs its left
    child's hash (a level-1 output) at level 2, then the right child's at level 3; the root at levels 4 and 5.  6 levels = 2 * height, holding
    4, 4, 2, 2, 1, 1 segments.
  * a two-block preimage (40 bytes: one full block and the padded last one): 2 segments at levels 0 and 1, n = 1,944."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import assembly_cases as AC

L = AC.L
FAKE = C.c_void_p(1)            # a context that is never dereferenced: every call below is refused before the device is needed


class StubProver(bpg.Prover):
    """Assembly-only prover; commitments are hash bytes made on the host (bpg_test_prover_stub_commitments)."""
    def __init__(self, ctx, transcript):
        super().__init__(None, transcript)
        self.test_stub_commitments()


class Api:
    Transcript, Prover = bpg.Transcript, StubProver
    BoundsCheck, MimcHash256, MerkleTree256 = bpg.BoundsCheck, bpg.MimcHash256, bpg.MerkleTree256
    commit, commit_all_single = staticmethod(bpg.commit), staticmethod(bpg.commit_all_single)
    mimc_hash, be_to_scalar = staticmethod(bpg.mimc_hash), staticmethod(bpg.be_to_scalar)


PROGRAM_CASES = [k for k, c in AC.CASES.items() if c["kind"] in ("mimc", "merkle")]


def _ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def evaluate(inst, prog):
    """the program read independently: Python integers mod l, from the committed values alone"""
    coef, v = _ints(inst.coef), [x % L for x in _ints(inst.v)]
    vals = ([], [], [], v)
    for i in range(inst.n):
        lr = []
        for a, b in ((prog.lc_ptr[2 * i], prog.lc_ptr[2 * i + 1]), (prog.lc_ptr[2 * i + 1], prog.lc_ptr[2 * i + 2])):
            acc = 0
            for k in range(int(a), int(b)):
                kind, idx = int(prog.term_var[k]) >> 29, int(prog.term_var[k]) & 0x1fffffff
                assert kind == 4 or kind == 3 or idx < i, "a multiplier may read only earlier multipliers"
                acc += coef[prog.term_coef[k]] * (1 if kind == 4 else vals[kind][idx])
            lr.append(acc % L)
        vals[0].append(lr[0]); vals[1].append(lr[1]); vals[2].append(lr[0] * lr[1] % L)
    return vals[0], vals[1], vals[2]


@pytest.mark.parametrize("name", PROGRAM_CASES)
def test_program_reproduces_the_host_assembly(name):
    p, _, _ = AC.build(Api, name)
    inst, prog = p.instance(), p.witness_program()
    assert len(prog.lc_ptr) == 2 * inst.n + 1 and prog.lc_ptr[0] == 0 and len(prog.term_var) == len(prog.term_coef) == prog.lc_ptr[-1]
    aL, aR, aO = evaluate(inst, prog)
    assert (aL, aR, aO) == (_ints(inst.aL), _ints(inst.aR), _ints(inst.aO))
    # ... and the device's interpreter, compiled for the host, over the packed and scheduled form of the same program
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    cs, cp = inst.cstruct(), prog.cstruct()
    assert bpg.lib().bpg_test_template_eval(C.byref(cs), C.byref(cp), inst.v, *out) == 0, bpg.lib().bpg_last_error()
    assert (out[0].raw, out[1].raw, out[2].raw) == (inst.aL, inst.aR, inst.aO)


def test_unreduced_committed_value_on_the_host_interpreter():
    """Scalar::from_bits range: a committed value >= l gives the host assembly's witness"""
    t = bpg.Transcript(b"MerkleTree"); p = StubProver(None, t)
    big = [((L + 5 + i) | (1 << 254)).to_bytes(32, "little") for i in range(2)]
    assert all(int.from_bytes(b, "little") >= L for b in big)
    vs = [p.commit(b, bytes(32))[1] for b in big]
    bpg.MerkleTree256(bytes(32), [], bpg.vars_to_lc(vs), "(W W)").prove(p, [], [])
    inst, prog = p.instance(), p.witness_program()
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    cs, cp = inst.cstruct(), prog.cstruct()
    assert bpg.lib().bpg_test_template_eval(C.byref(cs), C.byref(cp), b"".join(big), *out) == 0
    assert (out[0].raw, out[1].raw, out[2].raw) == (inst.aL, inst.aR, inst.aO)


def schedule(inst, prog):
    cs, cp = inst.cstruct(), prog.cstruct()
    buf = C.create_string_buffer(1 << 20)
    assert bpg.lib().bpg_test_template_schedule(C.byref(cs), C.byref(cp), buf, C.c_uint64(len(buf))) == 0, bpg.lib().bpg_last_error()
    return json.loads(buf.value.decode())


def check_invariant(inst, prog, S):
    first, level = S["seg_first"], S["seg_level"]
    assert first[0] == 0 and first[-1] == inst.n and all(a < b for a, b in zip(first, first[1:])), "segments partition [0, n)"
    assert len(level) == len(first) - 1 == S["segments"] and S["levels"] == max(level) + 1 <= S["max_levels"]
    seg_of = np.repeat(np.arange(len(level)), np.diff(first))
    for s in range(len(level)):
        a, b = int(prog.lc_ptr[2 * first[s]]), int(prog.lc_ptr[2 * first[s + 1]])
        tv = prog.term_var[a:b]
        ext = tv[((tv >> 29) <= 2) & ((tv & 0x1fffffff) < first[s])] & 0x1fffffff
        assert all(level[seg_of[i]] < level[s] for i in ext), "an external reference points to a lower level"
    assert S["level_segments"] == [level.count(l) for l in range(S["levels"])]


@pytest.mark.parametrize("name", PROGRAM_CASES)
def test_schedule_invariant(name):
    p, _, _ = AC.build(Api, name)
    inst, prog = p.instance(), p.witness_program()
    check_invariant(inst, prog, schedule(inst, prog))


def test_schedule_counts_derived_by_hand():
    a = workloads.merkle_full_tree(None, leaves=8, seed=1, prover_cls=StubProver)
    inst, prog = a.prover.instance(), a.prover.witness_program()
    S = schedule(inst, prog)
    check_invariant(inst, prog, S)
    assert inst.n == 13608 and S["segments"] == 14 and S["levels"] == 6 and S["level_segments"] == [4, 4, 2, 2, 1, 1]
    assert all(b - a == 972 for a, b in zip(S["seg_first"], S["seg_first"][1:]))
    a = workloads.mimc_preimage(None, nbytes=40, seed=1, prover_cls=StubProver)
    inst, prog = a.prover.instance(), a.prover.witness_program()
    S = schedule(inst, prog)
    check_invariant(inst, prog, S)
    assert inst.n == 1944 and S["segments"] == 2 and S["levels"] == 2 and S["seg_level"] == [0, 1] and S["seg_first"] == [0, 972, 1944]


def _err():
    return (bpg.lib().bpg_last_error() or b"").decode()


def _small():
    a = workloads.mimc_preimage(None, nbytes=40, seed=2, prover_cls=StubProver)
    return a.prover, a.prover.instance(), a.prover.witness_program()


def test_free_multipliers_are_refused():
    a = workloads.bounds_check_64(None, seed=1, prover_cls=StubProver)
    with pytest.raises(bpg.BpgError) as e:
        a.prover.witness_program()
    assert e.value.status == 4 and "free multiplier" in str(e.value)
    with pytest.raises(bpg.BpgError) as e:
        a.prover.template(None)                                         # refused before the (missing) context matters
    assert e.value.status == 4
    empty = StubProver(None, bpg.Transcript(b"empty"))
    with pytest.raises(bpg.BpgError) as e:
        empty.witness_program()
    assert e.value.status == 4 and "no multipliers" in str(e.value)


def test_upload_template_refusals_need_no_device():
    lib = bpg.lib()
    p, inst, prog = _small()
    cs, cp = inst.cstruct(), prog.cstruct()
    h = C.c_void_p(7)
    assert lib.bpg_r1cs_upload_template(None, C.byref(cs), C.byref(cp), C.byref(h)) == 4 and not h.value
    assert lib.bpg_r1cs_upload_template(FAKE, None, C.byref(cp), C.byref(h)) == 4
    assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), None, C.byref(h)) == 4
    assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), C.byref(cp), None) == 4
    # a term that refers forward (multiplier 5 reads its own output), and one past the committed values
    k = int(prog.lc_ptr[10])
    for bad, word in ((2 << 29 | 5, "earlier"), (2 << 29 | (inst.n - 1), "earlier"), (3 << 29 | inst.m, "committed")):
        q = bpg.WitnessProgram(prog.lc_ptr, prog.term_var.copy(), prog.term_coef, prog.param_rows)
        q.term_var[k] = bad
        cq = q.cstruct()
        assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), C.byref(cq), C.byref(h)) == 4 and word in _err() and not h.value, _err()
    q = bpg.WitnessProgram(prog.lc_ptr, prog.term_var, prog.term_coef.copy(), prog.param_rows)
    q.term_coef[k] = inst.ncoef
    cq = q.cstruct()
    assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), C.byref(cq), C.byref(h)) == 4 and "coefficient" in _err()
    q = bpg.WitnessProgram(prog.lc_ptr.copy(), prog.term_var, prog.term_coef, prog.param_rows)
    q.lc_ptr[3] = q.lc_ptr[2] - 1 if q.lc_ptr[2] else q.lc_ptr[4] + 1
    cq = q.cstruct()
    assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), C.byref(cq), C.byref(h)) == 4
    for rows, word in (([inst.q], "out of range"), ([inst.q - 1, inst.q - 1], "twice")):
        q = bpg.WitnessProgram(prog.lc_ptr, prog.term_var, prog.term_coef, rows)
        cq = q.cstruct()
        assert lib.bpg_r1cs_upload_template(FAKE, C.byref(cs), C.byref(cq), C.byref(h)) == 4 and word in _err(), _err()


def test_a_long_dependent_chain_is_refused():
    """5000 multipliers, each reading a committed value of its own and its predecessor's output: 5000 levels of one segment (cap: 4096 launches)"""
    n = 5000
    inst = bpg.R1CSInstance()
    row_ptr, one = np.zeros(1, dtype=np.uint64), (1).to_bytes(32, "little")
    inst.n, inst.q, inst.m, inst.nnz, inst.ncoef = n, 0, n, 0, 1
    inst.row_ptr, inst.coef = row_ptr.ctypes.data, C.cast(C.c_char_p(one), C.c_void_p).value
    tv, ptr = [], [0]
    for i in range(n):
        tv += [3 << 29 | i] + ([2 << 29 | (i - 1)] if i else []); ptr.append(len(tv))
        tv += [3 << 29 | i]; ptr.append(len(tv))
    prog = bpg.WitnessProgram(ptr, tv, np.zeros(len(tv), dtype=np.uint32))
    cp = prog.cstruct()
    buf = C.create_string_buffer(1 << 20); h = C.c_void_p()
    assert bpg.lib().bpg_test_template_schedule(C.byref(inst), C.byref(cp), buf, C.c_uint64(len(buf))) == 4 and "5000 dependent levels" in _err(), _err()
    assert bpg.lib().bpg_r1cs_upload_template(FAKE, C.byref(inst), C.byref(cp), C.byref(h)) == 4 and "levels" in _err() and not h.value
    inst.n = 0                                                            # no multipliers at all
    assert bpg.lib().bpg_r1cs_upload_template(FAKE, C.byref(inst), C.byref(cp), C.byref(h)) == 4 and "no multipliers" in _err()


def test_assign_refusals_need_no_device():
    lib = bpg.lib()
    p, inst, prog = _small()
    prog.param_rows = [inst.q - 1]
    cs, cp = inst.cstruct(), prog.cstruct()
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle(C.byref(cs), C.byref(cp), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 0, _err()
    v, par = bytes(32 * inst.m), bytes(32)
    m, one = C.c_uint64(inst.m), C.c_uint64(1)
    try:
        assert lib.bpg_r1cs_assign(FAKE, plain, m, v, C.c_uint64(0), None) == 4 and "not a template" in _err()
        assert lib.bpg_r1cs_assign(None, tmpl, m, v, one, par) == 4
        assert lib.bpg_r1cs_assign(FAKE, None, m, v, one, par) == 4
        assert lib.bpg_r1cs_assign(FAKE, tmpl, C.c_uint64(inst.m + 1), v + bytes(32), one, par) == 4 and "m does not match" in _err()
        assert lib.bpg_r1cs_assign(FAKE, tmpl, m, v, C.c_uint64(0), None) == 4 and "n_params" in _err()
        assert lib.bpg_r1cs_assign(FAKE, tmpl, m, v, C.c_uint64(2), par * 2) == 4 and "n_params" in _err()
        assert lib.bpg_r1cs_assign(FAKE, tmpl, m, None, one, par) == 4
        assert lib.bpg_r1cs_assign(FAKE, tmpl, m, v, one, None) == 4
        # a handle without device state is refused by everything that would launch
        ts = C.create_string_buffer(203); out = C.create_string_buffer(4096); ln = C.c_uint64(4096)
        assert lib.bpg_r1cs_assign(FAKE, tmpl, m, v, one, par) == 4 and "no device state" in _err()
        assert lib.bpg_r1cs_prove_resident(FAKE, tmpl, ts, m, v, bytes(32), C.c_uint32(0), out, C.byref(ln), None) == 4
        assert lib.bpg_r1cs_verify_resident(FAKE, tmpl, ts, m, v, bytes(64), C.c_uint64(64), bytes(32), C.c_uint32(0)) == 4
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [a.strip() for a in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    assert proto("bpg_r1cs_upload_template") == ["bpg_ctx *ctx", "const bpg_r1cs_instance *inst", "const bpg_witness_program *program", "bpg_circuit **out"]
    assert proto("bpg_r1cs_assign") == ["bpg_ctx *ctx", "bpg_circuit *c", "uint64_t m", "const uint8_t *v", "uint64_t n_params", "const uint8_t *param_values"]
    assert proto("bpg_prover_witness_program") == ["bpg_prover *p", "bpg_witness_program *out"]
    assert [f for f, _ in bpg.WitnessProgramView._fields_] == ["lc_ptr", "term_var", "term_coef", "n_params", "param_rows"]
    assert "bpg_witness_program" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)         # listed with the frozen structs
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_upload_template", "bpg_r1cs_assign", "bpg_prover_witness_program", "bpg_prover_mark_param_row"))
    p, inst, prog = _small()
    p.mark_param_row(inst.q - 1)
    assert p.witness_program().param_rows == [inst.q - 1]
    with pytest.raises(bpg.BpgError):
        p.mark_param_row(inst.q - 1)                                      # twice
    with pytest.raises(bpg.BpgError):
        p.mark_param_row(inst.q)
