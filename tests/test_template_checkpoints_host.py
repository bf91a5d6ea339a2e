"""Checkpointed circuit templates without a GPU: the schedule and the packed program with checkpoints, the notes a prover keeps, and the device's
interpreter compiled for the host (bpg_test_template_eval_checkpointed: poisoned vectors, the segments of every level in reverse order, then the verify step).

The yardstick is the prover's own host assembly (instance()); the checkpoint VALUES never come from it: Python integers for the chain, the native host
sponge for the hash circuits (checkpoint_cases.py).

Level and segment counts, from the cutting rule of host/template.hpp (a multiplier that names a committed value or a checkpoint its segment has not named
opens a segment; a checkpoint read adds no level):
  * chain: every block names a committed value of its own -> 6 segments; block k reads block k - 1's output -> 6 levels; with the five outputs
    checkpointed nothing reads another segment -> 1 level.
  * 3-block preimage: 3 segments at levels 0, 1, 2; every state checkpointed -> 1 level.
  * a path node absorbs two children: block 1 reads block 0's state (never checkpointed: the tree does not store it) -> with every node digest
    checkpointed each node is a segment at level 0 and one at level 1 -> exactly 2 levels at any depth.  (Without: depth + 1 = 4 at index 0, where a node's
    first block continues the segment that made its left child, and more at the other indices.)
  * ((W W)(W W)): 4 levels without, 2 with the three node digests."""
import ctypes as C
import hashlib
import json
import struct

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import assembly_cases as AC
import pyref_r1cs as PR
import checkpoint_cases as CK

L = bpg.L
FAKE = C.c_void_p(1)            # a context that is never dereferenced: every call below is refused before the device is needed


class StubProver(bpg.Prover):
    """Assembly-only prover; commitments are hash bytes made on the host (bpg_test_prover_stub_commitments)."""
    def __init__(self, ctx, transcript):
        super().__init__(None, transcript)
        self.test_stub_commitments()


def _err():
    return (bpg.lib().bpg_last_error() or b"").decode()


def _views(inst, prog, hints, ck_vars):
    cs, cp = inst.cstruct(), prog.cstruct()
    ch = hints.cstruct() if hints is not None and len(hints) else None
    ck = bpg._checkpoints_cstruct(ck_vars)
    return cs, cp, ch, ck


def schedule_ck(inst, prog, hints, ck_vars, raw=False):
    cs, cp, ch, ck = _views(inst, prog, hints, ck_vars)
    buf = C.create_string_buffer(1 << 20)
    st = bpg.lib().bpg_test_template_schedule_checkpointed(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck), buf, C.c_uint64(len(buf)))
    assert st == 0, _err()
    return buf.value if raw else json.loads(buf.value.decode())


def eval_ck(inst, prog, hints, ck_vars, ck_values, v=None):
    """-> (a_L, a_R, a_O, first mismatch or None)"""
    cs, cp, ch, ck = _views(inst, prog, hints, ck_vars)
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    first = C.c_uint64(12345)
    st = bpg.lib().bpg_test_template_eval_checkpointed(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck), inst.v if v is None else v,
                                                       b"".join(ck_values) if ck_values else None, *out, C.byref(first))
    assert st == 0, _err()
    return out[0].raw, out[1].raw, out[2].raw, None if first.value == 2**64 - 1 else first.value


def packed(inst, prog, hints, ck_vars):
    cs, cp, ch, ck = _views(inst, prog, hints, ck_vars)
    words = C.c_uint64()
    args = (C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck))
    assert bpg.lib().bpg_test_template_packed(*args, None, C.c_uint64(0), C.byref(words)) == 0, _err()
    out = np.zeros(max(words.value, 1), np.uint32)
    assert bpg.lib().bpg_test_template_packed(*args, C.c_void_p(out.ctypes.data), C.c_uint64(words.value), C.byref(words)) == 0, _err()
    return out[:words.value]


def program(a):
    prog, hints = a.prover.witness_program(hints=True)
    return a.prover.instance(), prog, hints


def witness(inst):
    return inst.aL, inst.aR, inst.aO


# ------------------------------------------------------------------------------------------------ the hand-built chain
def test_chain_levels_and_witness():
    a = CK.chain(None, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    assert inst.n == 36 and len(a.ck_vars) == 5
    S0 = schedule_ck(inst, prog, hints, [])
    assert S0["levels"] == 6 and S0["segments"] == 6 and S0["seg_level"] == [0, 1, 2, 3, 4, 5]
    S = schedule_ck(inst, prog, hints, a.ck_vars)
    assert S["levels"] == 1 and S["segments"] == 6 and S["level_segments"] == [6] and S["seg_first"] == [0, 6, 12, 18, 24, 30, 36]
    aL, aR, aO, first = eval_ck(inst, prog, hints, a.ck_vars, a.ck_values)
    assert first is None and (aL, aR, aO) == witness(inst)
    # the values are the circuit's own outputs at the named variables, and were computed without it
    assert [inst.aO[32 * v.index:32 * v.index + 32] for v in a.ck_vars] == a.ck_values
    # every term that names a checkpoint is packed as kind 5 with the position in the list; nothing else is
    stream, plain = packed(inst, prog, hints, a.ck_vars), packed(inst, prog, hints, [])
    assert len(stream) == len(plain)
    diff = np.nonzero(stream != plain)[0]
    assert len(diff) and all(int(plain[i]) in [int(v) for v in a.ck_vars] for i in diff)
    assert all(int(stream[i]) == (5 << 29 | [int(v) for v in a.ck_vars].index(int(plain[i]))) for i in diff)
    named = sum(int(np.count_nonzero(prog.term_var == int(v))) for v in a.ck_vars)
    assert named == 10 and len(diff) == 5         # block k's first round reads the link in both lists of t * t, and the packer writes the list once (SAME_AS_LEFT)


def test_an_empty_checkpoint_set_changes_nothing():
    a = CK.chain(None, seed=2, prover_cls=StubProver)
    inst, prog, hints = program(a)
    cs, cp = inst.cstruct(), prog.cstruct()
    buf = C.create_string_buffer(1 << 20)
    assert bpg.lib().bpg_test_template_schedule(C.byref(cs), C.byref(cp), buf, C.c_uint64(len(buf))) == 0, _err()
    assert schedule_ck(inst, prog, hints, [], raw=True) == buf.value
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    assert bpg.lib().bpg_test_template_eval(C.byref(cs), C.byref(cp), inst.v, *out) == 0, _err()
    aL, aR, aO, first = eval_ck(inst, prog, hints, [], [])
    assert first is None and (aL, aR, aO) == (out[0].raw, out[1].raw, out[2].raw) == witness(inst)
    # NULL checkpoints are the empty set
    st = bpg.lib().bpg_test_template_schedule_checkpointed(C.byref(cs), C.byref(cp), None, None, buf, C.c_uint64(len(buf)))
    assert st == 0 and json.loads(buf.value.decode())["levels"] == 6


# ------------------------------------------------------------------------------------------------ MimcHash256, MerkleTree256
def test_preimage_notes_levels_and_witness():
    a = CK.preimage3(None, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    assert inst.n == 2916
    notes = a.prover.noted()
    assert len(notes) == 3 and [b for _, b, _ in notes] == [0, 1, 2] and [last for _, _, last in notes] == [False, False, True]
    assert [(v.kind, v.index) for v, _, _ in notes] == [(2, 971), (2, 1943), (2, 2915)]
    assert schedule_ck(inst, prog, hints, [])["levels"] == 3
    S = schedule_ck(inst, prog, hints, a.ck_vars)
    assert S["levels"] == 1 and S["segments"] == 3
    aL, aR, aO, first = eval_ck(inst, prog, hints, a.ck_vars, a.ck_values)
    assert first is None and (aL, aR, aO) == witness(inst)
    assert a.ck_values[-1] == bpg.mimc_sponge([inst.v[0:32], inst.v[32:64], inst.v[96:128]]) == inst.aO[-32:]


@pytest.mark.parametrize("index", range(8))
def test_merkle_path_two_levels(index):
    a = CK.path(None, index, depth=3, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    assert inst.n == 5832 and inst.m == 4
    notes = a.prover.noted()
    assert [(b, last) for _, b, last in notes] == [(0, False), (1, True)] * 3
    # the note order is the bottom-up path order: the k-th digest is the ancestor k + 1 levels above the leaf
    assert [inst.aO[32 * v.index:32 * v.index + 32] for v in a.ck_vars] == a.ck_values and a.ck_values[-1] == a.root
    assert schedule_ck(inst, prog, hints, [])["levels"] >= 4         # depth + 1 when the path always continues on the left (index 0), more otherwise
    S = schedule_ck(inst, prog, hints, a.ck_vars)
    assert S["levels"] == 2 and S["segments"] == 6 and S["level_segments"] == [3, 3]
    aL, aR, aO, first = eval_ck(inst, prog, hints, a.ck_vars, a.ck_values)
    assert first is None and (aL, aR, aO) == witness(inst)


def test_merkle_path_pattern():
    assert workloads.merkle_path_pattern(0, 2) == ("((W W) W)", [("leaf", None), ("sibling", 0), ("sibling", 1)])
    assert workloads.merkle_path_pattern(1, 2) == ("((W W) W)", [("sibling", 0), ("leaf", None), ("sibling", 1)])
    assert workloads.merkle_path_pattern(2, 2) == ("(W (W W))", [("sibling", 1), ("leaf", None), ("sibling", 0)])
    assert workloads.merkle_path_pattern(5, 3) == ("(W ((W W) W))", [("sibling", 2), ("sibling", 0), ("leaf", None), ("sibling", 1)])


def test_full_tree_of_four_leaves():
    a = CK.full_tree4(None, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    assert len(a.ck_vars) == 3 and a.ck_values[-1] == a.root
    assert schedule_ck(inst, prog, hints, [])["levels"] == 4
    S = schedule_ck(inst, prog, hints, a.ck_vars)
    assert S["levels"] == 2 and S["level_segments"] == [3, 3]
    aL, aR, aO, first = eval_ck(inst, prog, hints, a.ck_vars, a.ck_values)
    assert first is None and (aL, aR, aO) == witness(inst)


def test_sponge_states():
    blocks = [workloads.synth("ck-states", i, 32) for i in range(4)]            # any 256-bit value
    states = bpg.mimc_sponge_states(blocks)
    assert states == [bpg.mimc_sponge(blocks[:k + 1]) for k in range(4)]
    assert bpg.lib().bpg_mimc_sponge_states(None, C.c_uint64(1), C.create_string_buffer(32)) == 4
    assert bpg.lib().bpg_mimc_sponge_states(blocks[0], C.c_uint64(0), C.create_string_buffer(32)) == 4


# ------------------------------------------------------------------------------------------------ mismatches
def test_mismatch_reporting():
    a = CK.chain(None, seed=3, prover_cls=StubProver)
    inst, prog, hints = program(a)
    wrong = lambda b: bpg.scalar_op("add", b, bpg.scalar_from_int(1))
    for k in range(5):
        vals = list(a.ck_values); vals[k] = wrong(vals[k])
        assert eval_ck(inst, prog, hints, a.ck_vars, vals)[3] == k
    vals = list(a.ck_values); vals[3] = wrong(vals[3]); vals[1] = wrong(vals[1])
    assert eval_ck(inst, prog, hints, a.ck_vars, vals)[3] == 1
    # x + l, where it is below 2^255, is the same scalar: accepted, and the witness is the same
    plus_l = [k for k, b in enumerate(a.ck_values) if int.from_bytes(b, "little") + L < 1 << 255]
    assert plus_l, "the seed gives no value with room for + l"
    vals = list(a.ck_values)
    for k in plus_l:
        vals[k] = (int.from_bytes(vals[k], "little") + L).to_bytes(32, "little")
    aL, aR, aO, first = eval_ck(inst, prog, hints, a.ck_vars, vals)
    assert first is None and (aL, aR, aO) == witness(inst)
    # the committed values of another witness under these checkpoints: block 0's output is not checkpoint 0
    other = CK.chain(None, seed=4, prover_cls=StubProver).prover.instance()
    assert eval_ck(inst, prog, hints, a.ck_vars, a.ck_values, v=other.v)[3] == 0


def test_a_forgotten_redirect_would_show():
    """what the hook is for: with the link of block 2 left out of the checkpoint list, block 2's segment is one level above block 1's and reads its output -
    in reverse order within a level that is only right because the schedule says so; the witness still matches, the levels do not collapse"""
    a = CK.chain(None, seed=5, prover_cls=StubProver)
    inst, prog, hints = program(a)
    some = [a.ck_vars[0]] + a.ck_vars[2:]
    S = schedule_ck(inst, prog, hints, some)
    assert S["levels"] == 2 and S["seg_level"] == [0, 0, 1, 0, 0, 0]
    aL, aR, aO, first = eval_ck(inst, prog, hints, some, [a.ck_values[0]] + a.ck_values[2:])
    assert first is None and (aL, aR, aO) == witness(inst)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    lib = bpg.lib()
    a = CK.chain(None, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    good = [int(v) for v in a.ck_vars]
    buf = C.create_string_buffer(1 << 16); h = C.c_void_p(7)
    for bad, word in ((good[:2] + [2 << 29 | inst.n], "out of range"), (good[:2] + [good[0]], "already"), (good + [3 << 29 | 0], "no multiplier variable"),
                      (good + [4 << 29], "no multiplier variable")):
        cs, cp, ch, ck = _views(inst, prog, hints, bad)
        assert lib.bpg_test_template_schedule_checkpointed(C.byref(cs), C.byref(cp), None, C.byref(ck), buf, C.c_uint64(len(buf))) == 4 and word in _err(), _err()
        assert lib.bpg_r1cs_upload_template_checkpointed(FAKE, C.byref(cs), C.byref(cp), None, C.byref(ck), C.byref(h)) == 4 and word in _err() and not h.value, _err()
    cs, cp, ch, ck = _views(inst, prog, hints, good)
    ck.vars = None
    assert lib.bpg_r1cs_upload_template_checkpointed(FAKE, C.byref(cs), C.byref(cp), None, C.byref(ck), C.byref(h)) == 4 and "vars" in _err()
    assert bpg.STATUS_NAMES[9] == "CHECKPOINT_MISMATCH" and lib.bpg_strerror(9) == b"checkpoint mismatch"
    # the assign calls on a handle without device state: count checks first, then "no device state"
    cs, cp, ch, ck = _views(inst, prog, hints, good)
    assert lib.bpg_test_circuit_handle(C.byref(cs), C.byref(cp), C.byref(h)) == 0, _err()
    try:
        first = C.c_uint64(5)
        m, v = C.c_uint64(inst.m), inst.v
        assert lib.bpg_r1cs_assign_checkpointed(FAKE, h, m, v, C.c_uint64(0), None, C.c_uint64(5), b"".join(a.ck_values), C.byref(first)) == 4 and "n_ck" in _err()
        assert first.value == 2**64 - 1
        assert lib.bpg_r1cs_assign_checkpointed(FAKE, h, m, v, C.c_uint64(0), None, C.c_uint64(0), None, None) == 4 and "no device state" in _err()
    finally:
        lib.bpg_r1cs_free(None, h)


def test_header_and_binding():
    import re
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "bpg_witness_checkpoints" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)
    assert re.search(r"#define BPG_ERR_CHECKPOINT_MISMATCH 9\b", hdr) and re.search(r"#define BPG_ABI_VERSION 7u", hdr)
    assert [f for f, _ in bpg.WitnessCheckpointsView._fields_] == ["n_checkpoints", "vars"]
    assert re.search(r"uint64_t n_checkpoints;\s*const uint32_t \*vars;", hdr)


# ------------------------------------------------------------------------------------------------ noting changes no byte
class HostProver(bpg.Prover):
    """Assembly-only prover whose Pedersen commitments come from the CPU oracle (as tests/test_assembly_fixtures.py has it)."""
    def __init__(self, ctx, transcript):
        super().__init__(None, transcript)

    def commit(self, v, v_blinding):
        com = O.pedersen_commit((int.from_bytes(v, "little") % L).to_bytes(32, "little"), v_blinding)
        return com, self.commit_precomputed(v, v_blinding, com)

    def commit_many(self, vs, blindings):
        out = [self.commit(v, b) for v, b in zip(vs, blindings)]
        return [c for c, _ in out], [x for _, x in out]


class ProductApi:
    Transcript, Prover = bpg.Transcript, HostProver
    BoundsCheck, MimcHash256, MerkleTree256 = bpg.BoundsCheck, bpg.MimcHash256, bpg.MerkleTree256
    commit, commit_single, commit_all_single = staticmethod(bpg.commit), staticmethod(bpg.commit_single), staticmethod(bpg.commit_all_single)
    mimc_hash, be_to_scalar = staticmethod(bpg.mimc_hash), staticmethod(bpg.be_to_scalar)


@pytest.fixture
def setup_without_a_device(monkeypatch):
    def setup(self, prover, witnesses, blindings):
        derived = self.preprocess(witnesses)
        coms, out = [], []
        for s, b in zip(derived, blindings):
            com, v = prover.commit(s, b)
            coms.append(com); out.append((s, v))
        return coms, out
    monkeypatch.setattr(bpg.Gadget, "setup", setup)


FIX = json.loads((O.ROOT / "tests" / "golden" / "assembly.json").read_text())


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_noting_changes_no_byte(name, setup_without_a_device):
    """every circuit of assembly_cases.py against tests/golden/assembly.json: the digests of instance(), of the committed values and of the transcript are
    the recorded ones, whether or not the gadgets of the circuit note anything.  (The file's remaining entry, example_gadgets, goes through the file driver:
    tests/test_assembly_fixtures.py checks it, unchanged.)"""
    p, t, coms = AC.build(ProductApi, name)
    inst, want = p.instance(), FIX[name]
    rp = struct.unpack("<%dQ" % (inst.q + 1), inst.row_ptr)
    tv, tc = struct.unpack("<%dI" % rp[-1], inst.term_var), struct.unpack("<%dI" % rp[-1], inst.term_coef)
    coef = [int.from_bytes(inst.coef[32 * i:32 * i + 32], "little") for i in range(len(inst.coef) // 32)]
    rows = ([(tv[k], coef[tc[k]]) for k in range(rp[r], rp[r + 1])] for r in range(inst.q))
    ints = lambda b: [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]
    assert (inst.n, inst.q, inst.m) == (want["n"], want["q"], want["m"])
    assert PR.digest_rows(rows) == want["constraints_sha256"]
    assert PR.digest_scalars(ints(inst.aL), ints(inst.aR), ints(inst.aO)) == want["witness_sha256"]
    assert PR.digest_scalars(ints(inst.v), ints(inst.v_blinding)) == want["committed_sha256"]
    assert hashlib.sha256(t.state).hexdigest() == want["transcript_state_sha256"]
    assert [c.hex() for c in coms] == want["commitments"]
    notes = p.noted()
    assert bool(notes) == (AC.CASES[name]["kind"] in ("mimc", "merkle")), "the sponge gadgets note their states; nothing else does"
    assert all(v.kind == 2 for v, _, _ in notes)


def test_range_proof_over_a_checkpointed_hash_output():
    """a 64-bit range proof whose source is the (checkpointed) digest of a two-block sponge: the hints still pack, their source is read as kind 5, and the
    bits are those of the caller's value"""
    t = bpg.Transcript(b"RangeOverHash"); p = StubProver(None, t)
    blocks = [bpg.scalar_from_int(5), bpg.scalar_from_int(9)]
    coms, vs = p.commit_many(blocks, [bytes(32)] * 2)
    g = bpg.MerkleTree256(bpg.mimc_sponge(blocks), [], bpg.vars_to_lc(vs), "(W W)")
    g.prove(p, [], [])
    out = [v for v, _, last in p.noted() if last]
    assert len(out) == 1
    value = bpg.mimc_sponge(blocks)
    bpg.range_proof(p, bpg.LinearCombination.of(out[0]), 64, value)
    prog, hints = p.witness_program(hints=True)
    inst = p.instance()
    assert inst.n == 1944 + 64 and len(hints) == 64
    stream = packed(inst, prog, hints, out)
    first_hint = int(hints.mul[0])
    assert first_hint == 1944
    # the record of the first hinted multiplier: one source term, of kind 5, position 0
    S = schedule_ck(inst, prog, hints, out)
    assert S["seg_first"][-2] == 1944 and S["seg_level"][-1] == 0, "the range reads the caller's value: level 0, not one above the sponge"
    plain = packed(inst, prog, hints, [])
    diff = np.nonzero(stream != plain)[0]
    assert len(diff) == 1 and int(plain[diff[0]]) == int(out[0]) and int(stream[diff[0]]) == 5 << 29
    aL, aR, aO, first = eval_ck(inst, prog, hints, out, [value])
    assert first is None and (aL, aR, aO) == witness(inst)
