"""The shape catalogue (tests/shape_cases.py) without a device: every case is the case it says it is, the oracle proves and verifies it, the integer model of
flattened_constraints(z) is tied to the ORACLE's proofs (not only to itself), and the size rule of the transposition workspace (csrc/host/csc_work.hpp) holds
on every (nvar, q) the GPU tests will send - where the lockstep wave's earlier layout, replayed by the same program, does not."""
import ctypes as C
import subprocess

import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import script_cases as S
import shape_cases as H

L = H.L
DEVICE_ERROR = 7


def test_names_are_unique_and_every_case_is_what_it_says():
    names = H.names()
    assert len(set(names)) == len(names) == 26
    for case in H.catalogue():
        assert case.predicate(case.circuit), case.name
        assert case.circuit.inst.q == H.q_of(case.circuit) and case.circuit.inst.nnz == H.nnz_of(case.circuit), case.name
    groups = {c.group for c in H.catalogue()}
    assert groups == {"tall", "wide", "empty", "const", "hot", "dup", "sect", "edge"}
    # the largest case has 2100 rows, or 700 multipliers; nothing needs more generators than the shared context holds
    assert max(H.q_of(c.circuit) for c in H.catalogue()) == 2100 and max(c.circuit.n for c in H.catalogue()) == 700
    assert max(c.circuit.N for c in H.catalogue()) <= H.GENS_CAPACITY
    assert [c.name for c in H.catalogue() if c not in H.lockstep_cases()] == ["tall/n0-m2-q300"]


def test_tall_waves_outgrow_the_old_layout():
    """the tall predicate, applied to the wave the lockstep test sends (K copies of the case), implies that the second scan's scratch ran past the `counts` the
    wave used to lay out, rounding included - from the sizes, not by hand.  The cases that are not tall stayed inside it, so they never showed it"""
    tall = [c for c in H.lockstep_cases() if H.is_tall(c.circuit)]
    assert {c.name for c in tall} >= {"tall/n1-q70", "tall/n3-m2-q600", "tall/n1-m1-q2100", "hot/aL0", "hot/v-last"}
    for case in H.lockstep_cases():
        over = H.scan_scratch_overrun([case.circuit] * H.LOCKSTEP_K)
        if H.is_tall(case.circuit):
            assert over > 0, case.name
            KN, qT, mT = H.wave_sizes([case.circuit] * H.LOCKSTEP_K)
            assert qT > 3 * KN + mT + 2
    # the issue's own example: eight copies of one multiplier under seventy rows write 560 words into a 256-byte block
    assert H.scan_scratch_overrun([H.by_name("tall/n1-q70").circuit] * 8) == 4 * 560 - 256


def wave_pairs():
    """(nvar, q) of everything the GPU tests transpose: every case alone, K copies of every lockstep case, the mixed waves by padded size, the repeats and joins"""
    pairs = {(H.nvar_of(c.circuit), H.q_of(c.circuit)) for c in H.catalogue()}
    by_N = {}
    for case in H.lockstep_cases():
        KN, qT, mT = H.wave_sizes([case.circuit] * H.LOCKSTEP_K)
        pairs.add((3 * KN + mT, qT))
        by_N.setdefault(case.circuit.N, []).append(case.circuit)
    for group in by_N.values():
        KN, qT, mT = H.wave_sizes(group)
        pairs.add((3 * KN + mT, qT))
    return sorted(pairs)


def old_layout_overruns(nvar, q):
    """does the transposition overrun the wave's earlier layout (nvar + 2 words of counts, rounded to 256 bytes)?  Only the second scan's scratch can"""
    return 4 * q > H.al256(4 * (nvar + 2))


def test_size_rule_of_the_transposition_workspace(tmp_path):
    """tests/hostcheck/csc_work.cpp under ASan and UBSan (a stand-alone program: no preload, no device): the transposition's launches replayed into heap blocks
    of exactly csc_work_words() words stay inside them on every pair, where the scans disagree on which side is larger included; replayed against the layout
    the lockstep wave had before, they overrun `counts` on exactly the pairs the sizes say - the tall waves"""
    exe = tmp_path / "csc_work"
    src = O.ROOT / "tests" / "hostcheck" / "csc_work.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    pairs = wave_pairs() + [(0, 0), (0, 1), (1, 0), (2047, 2048), (2048, 2047), (2048, 2049), (2049, 2048), (4096, 4097), (3, 4096), (5000, 1)]
    assert any(H.scan_blocks(nv) > H.scan_blocks(q) for nv, q in pairs) and any(H.scan_blocks(nv) < H.scan_blocks(q) for nv, q in pairs)
    args = ["%d:%d" % p for p in pairs]
    r = subprocess.run([str(exe), "rule"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.split()[-1] == "ok" and r.stdout.count(" ok\n") == len(pairs)
    old = subprocess.run([str(exe), "old-wave"] + args, capture_output=True, text=True, timeout=120)
    assert old.stderr == ""
    lines = old.stdout.splitlines()[:-1]
    assert len(lines) == len(pairs)
    overran = {p for p, line in zip(pairs, lines) if "OVERRUN" in line}
    assert overran == {p for p in pairs if old_layout_overruns(*p)}
    assert all(" counts " in line and " starts " not in line for line in lines if "OVERRUN" in line)
    for case in H.lockstep_cases():
        if H.is_tall(case.circuit):
            KN, qT, mT = H.wave_sizes([case.circuit] * H.LOCKSTEP_K)
            assert (3 * KN + mT, qT) in overran, case.name
    assert old.returncode == len(overran) > 0 and old.stdout.split()[-1] == "FAILED"


def test_oracle_finds_every_case_satisfied():
    for case in H.catalogue():
        assert S.satisfied(case.circuit), case.name


@pytest.mark.parametrize("flags", [0, 3])
def test_oracle_proves_and_verifies_every_case(flags):
    for case in H.catalogue():
        proof, _ = H.reference(case.name, 0, flags)
        assert len(proof) == O.proof_size(case.circuit.n, flags), case.name
        assert H.oracle_verify(case.circuit, proof, flags) == 0, case.name


def test_oracle_rejects_the_pinned_tamper_of_every_case():
    """the statement with one constant (or coefficient) of its last non-empty row changed: the oracle's verifier rejects the honest proof, so the tamper the GPU
    test repeats is one the reference decides; only a circuit without any term has none"""
    for case in H.catalogue():
        rows = H.tampered_rows(case.circuit)
        assert (rows is None) == (H.nnz_of(case.circuit) == 0), case.name
        if rows is not None:
            assert H.oracle_verify(case.circuit, H.reference(case.name)[0], 0, rows) == O.ERR_VERIFY, case.name


def test_model_weights_fit_the_oracles_proofs():
    """The model is not its own judge: under a scripted transcript (every challenge a fixed filler value) the ORACLE's proof carries t(x), its blinding and the
    final a, b of the inner-product argument, and script_cases.skeleton predicts them from the model's w_L, w_R, w_O, w_V - so those four are the oracle's.
    w_c never enters a prover's scalar; it is pinned by the verification identity t_2 = w_c + <w_V, v> + delta(y, z), whose left side has just been tied to the
    oracle: exactly one w_c fits."""
    for case in H.catalogue():
        c = case.circuit
        script = S.filler_script(c.lgN, b"shape script")
        rc, proof, _ = O.prove(H.gens(), c.state, S.oracle_circuit(c), H.vb_of(c), S.SEED, O.FLAG_FAST_MSM, script=S.script_bytes(script))
        assert rc == 0, case.name
        y, z = script[0], script[1]
        sk = S.skeleton(c.n, c.m, c.rows, c.aL, c.aR, c.aO, c.vb, S.draws(c, S.SEED), script)
        got = S.proof_scalars(proof, 0)
        for field in ("t_x", "t_x_blinding", "a", "b"):
            assert got[field] == sk[field], (case.name, field)
        wL, wR, wO, wV, wc = H.model(c, z)
        assert (wL, wR, wO, wV, wc) == (sk["wL"], sk["wR"], sk["wO"], sk["wV"], sk["wc"])
        assert sk["t"][2] == (wc + S.ip(wV, c.v) + H.delta(c, y, z)) % L, case.name
        assert O.verify(H.gens(), c.state, S.oracle_circuit(c), c.V, proof, S.SEED, 0, script=S.script_bytes(script)) == 0, case.name


def test_model_at_the_edges_of_z():
    """z = 1 sums the coefficients of a column, z = l - 1 alternates their signs, and a circuit without constants has w_c = 0 at every z"""
    for case in H.catalogue():
        c = case.circuit
        for _, z in H.Z_VALUES:
            wL, wR, wO, wV, wc = H.model(c, z)
            assert len(wL) == len(wR) == len(wO) == c.n and len(wV) == c.m
            if H.kind_count(c, H.KIND_ONE) == 0:
                assert wc == 0
        wL = H.model(c, 1)[0]
        for i in range(c.n):
            assert wL[i] == sum(co for pv, co in H.terms_of(c) if pv == H.VC.var(H.KIND_L, i)) % L
    hot = H.by_name("hot/aL0").circuit
    assert H.model(hot, L - 1)[0][0] == sum((-1) ** (r + 1) * co for r, row in enumerate(hot.rows) for pv, co in row if pv == H.VC.var(H.KIND_L, 0)) % L


def test_template_parts_keep_the_rows():
    """the template form of a case (a program of constants) has the case's own rows, entry for entry, and its host-assembled repeat and join evaluate to the
    concatenated witnesses: what the GPU test compares a device-made repeat or join with is a satisfied circuit the oracle accepts"""
    tall, wide = H.by_name("tall/n1-q70").circuit, H.by_name("wide/q0-n2-m3").circuit
    for c in (tall, wide):
        inst, prog = H.template_parts(c)
        assert (inst.row_ptr == c.inst.row_ptr).all() and (inst.term_var == c.inst.term_var).all() and (inst.term_coef == c.inst.term_coef).all()
        assert inst.coef[:len(c.inst.coef)] == c.inst.coef and (inst.aL, inst.aR, inst.aO) == (c.inst.aL, c.inst.aR, c.inst.aO)
    inst, prog = H.template_parts(tall)
    rep = H.assembled("rep", b"Shape repeat", [(tall, 3)], bpg.test_template_repeat_instance(inst, prog, None, 3))
    assert (rep.n, rep.m, H.q_of(rep)) == (3, 0, 210) and S.satisfied(rep)
    winst, wprog = H.template_parts(wide)
    joined = H.assembled("join", b"Shape join", [(tall, 1), (wide, 1)], bpg.test_template_join_instance([(inst, prog, None, 1), (winst, wprog, None, 1)]))
    assert (joined.n, joined.m, H.q_of(joined)) == (3, 3, 70) and S.satisfied(joined)


def test_weights_hook_without_device_fails_loudly():
    """bpg_test_weights has no CPU path: without a context it is a DEVICE_ERROR, and nothing is written"""
    out = C.create_string_buffer(b"\x5a" * 64, 64)
    rc = bpg.lib().bpg_test_weights(None, None, H.le(1), out)
    assert rc == DEVICE_ERROR and b"device" in bpg.lib().bpg_last_error()
    assert out.raw == b"\x5a" * 64
    assert hasattr(bpg.ResidentCircuit, "test_weights")
