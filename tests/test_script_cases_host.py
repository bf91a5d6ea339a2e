"""The catalogue of scripted proofs (tests/script_cases.py) without a device: the scripted transcript of the library and of the oracle, the integer model
against the oracle for every case, the properties the GPU test relies on - each derived from the case by the model, never assumed from its name - and the
oracle's decisions on the tampered proofs."""
import collections

import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import script_cases as S

L = S.L
INVALID_ARGUMENT = 4
SIZE_SAMPLES = ("all/N1/2/flags0", "all/N1n0/2/flags3", "all/N2/l-1/flags0", "one/N8/x=0", "one/N64/u_6=2^252", "all/N512/1/flags0", "all/N1024/2/flags3")


def real_challenges(case, proof):
    """the Fiat-Shamir replay of a proof in Python, on the oracle's transcript primitives: y, z, u, x, w, u_1 .. u_lgN as the real transcript yields them"""
    c, compact = case.circuit, case.flags & 1
    t = O.Transcript(state=c.state)
    t.append_u64(b"m", c.m)
    at = 1 if compact else 0
    for k, label in enumerate((b"A_I1", b"A_O1", b"S1")):
        t.append(label, proof[at + 32 * k:at + 32 * k + 32])
    at += 96
    if not case.flags & 2:
        t.append(b"dom-sep", b"r1cs-1phase")
    for k, label in enumerate((b"A_I2", b"A_O2", b"S2")):
        t.append(label, bytes(32) if compact else proof[at + 32 * k:at + 32 * k + 32])
    at += 0 if compact else 96
    out = [t.challenge_scalar(b"y"), t.challenge_scalar(b"z")]
    for k, label in enumerate((b"T_1", b"T_3", b"T_4", b"T_5", b"T_6")):
        t.append(label, proof[at + 32 * k:at + 32 * k + 32])
    at += 160
    out += [t.challenge_scalar(b"u"), t.challenge_scalar(b"x")]
    for k, label in enumerate((b"t_x", b"t_x_blinding", b"e_blinding")):
        t.append(label, proof[at + 32 * k:at + 32 * k + 32])
    at += 96
    out.append(t.challenge_scalar(b"w"))
    t.append(b"dom-sep", b"ipp v1")
    t.append_u64(b"n", c.N)
    for k in range(c.lgN):
        t.append(b"L", proof[at:at + 32]); t.append(b"R", proof[at + 32:at + 64])
        at += 64
        out.append(t.challenge_scalar(b"u"))
    return out, t.state


# ---------------------------------------------------------------------------------------------------- the catalogue
def test_catalogue_holds_what_the_issue_lists():
    cases = S.catalogue()
    groups = collections.Counter(c.group for c in cases)
    # one position at a time: 8 positions at N = 8, five at N = 64, each with the eleven values and 0 where the position is not inverted
    assert groups["one"] == (4 * 11 + 4 * 12) + (3 * 11 + 2 * 12)
    for tag, positions in (("N8", S.position_names(3)), ("N64", ("y", "z", "x", "u_1", "u_6"))):
        c = S.base_circuit(tag)
        fill = S.filler_script(c.lgN)
        for p in positions:
            k = S.position_names(c.lgN).index(p)
            got = [x for x in cases if x.name.startswith("one/%s/%s=" % (tag, p))]
            assert sorted(x.script[k] for x in got) == sorted(S.V + ((0,) if p in S.MAY_BE_ZERO else ()))
            assert all(x.script[:k] + x.script[k + 1:] == fill[:k] + fill[k + 1:] for x in got)
    assert (S.base_circuit("N8").n, S.base_circuit("N8").m, S.base_circuit("N64").n) == (5, 2, 40)
    assert S.R_INV * 2**256 % L == 1 and (L - S.R_INV) * 2**256 % L == L - 1               # the Montgomery forms 1 and l - 1
    # all positions at once: 1, 2, l - 1 at every size, dialects 0 and 3 at every size
    shapes = {(x.circuit.N, x.circuit.n, x.script[0], x.flags) for x in cases if x.group == "all"}
    for N, n in ((1, 1), (1, 0), (2, 2), (8, 5), (64, 40), (512, 300), (1024, 700)):
        for v in (1, 2, L - 1):
            assert (N, n, v, 0) in shapes
        assert any(s[:2] == (N, n) and s[3] == 3 for s in shapes)
    assert all(len(set(x.script)) == 1 for x in cases if x.group == "all")
    assert groups["cancel"] == 12 and groups["witness"] == 4
    for x in cases:
        assert len(x.script) == 5 + x.circuit.lgN and all(0 <= s < L for s in x.script), x.name
        assert x.script[0] and all(x.script[5:]), x.name                                   # refusals are not catalogue entries
    # the inputs a hashed challenge never produces
    assert any(x.script[1] == 0 for x in cases) and any(x.script[3] == 0 for x in cases) and any(x.script[4] == 0 for x in cases)
    assert any(u * u % L == 1 for x in cases for u in x.script[5:])


@pytest.mark.parametrize("tag", ["N64", "N1024"])
def test_cancellations_cancel_exactly(tag):
    sk = {kind: S.case_skeleton(S.by_name("cancel/%s/%s" % (tag, kind))) for kind in S.CANCELLATIONS}
    n = S.base_circuit(tag).n
    base = S.case_skeleton(S.by_name("one/N64/y=2" if tag == "N64" else "all/N1024/2/flags0"))
    assert all(base["r0"]) and all(base["l1"]) and base["t"][1] and base["rounds"][0]["cL"] and any(base["lx"])        # none of it happens by itself
    assert sk["wO=y^i"]["r0"][0] == 0 and sk["wO=y^i"]["r0"][n - 1] == 0 and all(sk["wO=y^i"]["r0"][1:n - 1])
    assert sk["l1=0"]["l1"][0] == 0 and sk["l1=0"]["l1"][n - 1] == 0 and all(sk["l1=0"]["l1"][1:n - 1])
    for i in (0, n - 1):
        a, b = sk["sum=l"]["sum_l2"][i]
        assert a and b and a + b == L                                                       # canonical operands, integer sum exactly l
    assert sk["cL=0"]["rounds"][0]["cL"] == 0 and sk["cL=0"]["rounds"][0]["cR"] != 0
    assert sk["t1=0"]["t"][1] == 0 and all(sk["t1=0"]["t"][2:])
    assert sk["x=0"]["x"] == 0 and not any(sk["x=0"]["lx"]) and sk["x=0"]["t_x"] == 0 and sk["x=0"]["a"] == 0
    for kind in S.CANCELLATIONS:                                                            # the solved witnesses still satisfy their circuits
        assert S.case_satisfied("cancel/%s/%s" % (tag, kind)), kind


def test_witness_edges_reach_every_value():
    for x in S.catalogue():
        if x.group == "witness":
            for vec in (x.circuit.aL, x.circuit.aR, x.circuit.aO):
                assert set(vec) <= set(S.WITNESS_EDGES)
            assert {v for vec in (x.circuit.aL, x.circuit.aR, x.circuit.aO) for v in vec} == set(S.WITNESS_EDGES)
            assert not S.case_satisfied(x.name)                                             # prover-only
        else:
            assert S.case_satisfied(x.name), x.name


# ---------------------------------------------------------------------------------------------------- the model and the scripted oracle
def test_model_equals_the_oracle_on_every_case():
    for case in S.catalogue():
        proof, _ = S.reference(case.name)
        sk = S.case_skeleton(case)
        got = S.proof_scalars(proof, case.flags)
        for f in ("t_x", "t_x_blinding", "e_blinding", "a", "b"):
            assert got[f] == sk[f], "%s: %s of the oracle's proof is not the model's" % (case.name, f)


@pytest.mark.parametrize("name", SIZE_SAMPLES)
def test_scripted_oracle_reproduces_the_unscripted_bytes(name):
    case = S.by_name(name)
    c = case.circuit
    vb = b"".join(S.le(x) for x in c.vb)
    rc, plain, after = O.prove(S.gens(), c.state, S.oracle_circuit(c), vb, case.seed, case.flags | O.FLAG_FAST_MSM)
    assert rc == 0
    real, state = real_challenges(case, plain)
    assert state == after
    rc, scripted, after2 = O.prove(S.gens(), c.state, S.oracle_circuit(c), vb, case.seed, case.flags | O.FLAG_FAST_MSM, script=real)
    assert (rc, scripted, after2) == (0, plain, after)
    assert scripted != S.reference(name)[0]
    assert O.verify(S.gens(), c.state, S.oracle_circuit(c), c.V, plain, S.SEED, case.flags, script=real) == O.verify(S.gens(), c.state, S.oracle_circuit(c), c.V, plain, S.SEED, case.flags) == 0


def test_scripted_oracle_verifier_accepts_every_satisfied_case():
    for case in S.catalogue():
        want = 0 if S.case_satisfied(case.name) else O.ERR_VERIFY
        assert S.oracle_verify(case, S.reference(case.name)[0]) == want, case.name
    # and without the script the same bytes are not a proof
    for name in SIZE_SAMPLES:
        case = S.by_name(name)
        assert O.verify(S.gens(), case.circuit.state, S.oracle_circuit(case.circuit), case.circuit.V, S.reference(name)[0], S.SEED, case.flags) == O.ERR_VERIFY


# The oracle's decision on every tampered proof.  x = 0 takes A_I, A_O, S and every T_k out of the verification equation (their scalars are x^k times
# something), so a tampered T_1 is legitimately accepted there; w = 0 only drops the term w (t_x - a b), which the r-weighted half of the equation does not
# need.  Everything else is rejected.
ACCEPTED_TAMPERS = {"one/N8/x=0#T_1"}


def test_tampers_are_pinned_with_the_oracles_decision():
    names = [n for n, _, _ in S.tampers()]
    assert len(names) == len(S.TAMPER_BASES) * len(S.TAMPER_FIELDS) - 1 and "all/N1n0/2/flags0#L_0" not in names       # (lg N = 0: no L_0)
    for name, case, proof in S.tampers():
        assert S.oracle_verify(case, proof) == (0 if name in ACCEPTED_TAMPERS else O.ERR_VERIFY), name


def test_proof_under_one_script_is_rejected_under_another_y():
    """(at N = 1 the proof holds y^0 alone and no y can matter: there the oracle accepts, and the other script differs in z as well to be refused)"""
    for name in SIZE_SAMPLES + ("cancel/N64/x=0", "one/N8/z=0"):
        case = S.by_name(name)
        other = S.wrong_script(case)
        assert other[1:] == list(case.script[1:]) and other[0] != case.script[0]
        assert S.oracle_verify(case, S.reference(name)[0], other) == (0 if case.circuit.N == 1 else O.ERR_VERIFY), name
        if case.circuit.N == 1:
            assert S.oracle_verify(case, S.reference(name)[0], [other[0], other[1] + 1] + other[2:]) == O.ERR_VERIFY, name


def test_oracle_refuses_bad_scripts():
    case = S.by_name("one/N8/y=2")
    c = case.circuit
    for bad in bad_scripts(case):
        rc, _, _ = O.prove(S.gens(), c.state, S.oracle_circuit(c), b"".join(S.le(x) for x in c.vb), case.seed, O.FLAG_FAST_MSM, script=bad)
        assert rc == O.ERR_ARG
        assert O.verify(S.gens(), c.state, S.oracle_circuit(c), c.V, S.reference(case.name)[0], S.SEED, 0, script=bad) == O.ERR_ARG


# ---------------------------------------------------------------------------------------------------- the library's scripted transcript, no device
def bad_scripts(case):
    good = S.script_bytes(case.script)
    out = [good[:-1], good + [S.le(1)], [], [S.le(L)] + good[1:], good[:2] + [b"\xff" * 32] + good[3:], good[:7] + [S.le(L + 1)]]      # length, non-canonical
    out += [[bytes(32)] + good[1:]] + [good[:k] + [bytes(32)] + good[k + 1:] for k in range(5, len(good))]                                # y = 0, u_k = 0
    return out


@pytest.mark.parametrize("name", SIZE_SAMPLES)
def test_scripted_transcript_exports_the_state_of_an_unscripted_one(name):
    """bpg_test_verify_replay_scripted: the same operations with and without a script leave the same 203 bytes - the oracle prover's own state after -, the
    script is handed out in order, entry by entry, and without one the challenges are the real ones"""
    case = S.by_name(name)
    c = case.circuit
    proof, after = S.reference(name)
    st1, state1, ch1, used1 = bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof, S.SEED, case.flags, S.script_bytes(case.script))
    st0, state0, ch0, used0 = bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof, S.SEED, case.flags, None)
    assert (st1, st0) == (0, 0)
    assert state1 == state0 == after
    assert ch1 == S.script_bytes(case.script) and used1 == 5 + c.lgN
    real, state = real_challenges(case, proof)
    assert ch0 == real and used0 == 0 and state == after
    assert bpg.test_verify_replay(c.n, c.m, S.GENS_CAPACITY, c.state, proof, S.SEED, case.flags) == (0, False)


def test_script_is_consumed_in_order_up_to_where_the_replay_stops():
    case = S.by_name("one/N8/w=3")
    c = case.circuit
    proof = S.reference(case.name)[0]
    script = S.script_bytes(case.script)
    at = 192 + 64                                                                           # T_4 as the identity: the replay stops after y and z
    st, _, ch, used = bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof[:at] + bytes(32) + proof[at + 32:], S.SEED, 0, script)
    assert (st, used) == (3, 2) and ch == script[:2] + [bytes(32)] * 6
    st, _, ch, used = bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof[:-1], S.SEED, 0, script)     # a format error: nothing drawn
    assert (st, used) == (2, 0) and ch == [bytes(32)] * 8


def test_hooks_refuse_bad_scripts():
    case = S.by_name("one/N8/y=2")
    c = case.circuit
    proof = S.reference(case.name)[0]
    for bad in bad_scripts(case):
        with pytest.raises(bpg.BpgError) as e:
            bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof, S.SEED, 0, bad)
        assert e.value.status == INVALID_ARGUMENT and "scripted:" in str(e.value)
    good = S.script_bytes(case.script)
    for k in (1, 2, 3, 4):                                                                  # z, u, x, w may be zero
        st, _, ch, used = bpg.test_verify_replay_scripted(c.n, c.m, S.GENS_CAPACITY, c.state, proof, S.SEED, 0, good[:k] + [bytes(32)] + good[k + 1:])
        assert (st, used) == (0, 8) and ch[k] == bytes(32)
