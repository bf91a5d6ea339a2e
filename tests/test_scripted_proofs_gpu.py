"""Whole proofs under a scripted transcript (tests/script_cases.py), byte for byte against the scripted CPU oracle: every challenge y, z, u, x, w, u_1 .. u_lgN
is chosen by the test, through bpg_test_prove_scripted, bpg_test_prove_batch_scripted, bpg_test_verify_scripted and bpg_test_verify_batch_scripted - the
production entry points on a transcript that hands out the script.

Inside a proof the challenges are hash outputs, so the scalar kernels (hip/k_scalars.cuh, the scalar side of hip/k_ipa.cuh, hip/k_verify.cuh) and the lockstep
wave (hip/k_batch.cuh) only ever see uniformly random 252-bit numbers.  Here they get 1, 2, l - 1, 2^252, the Montgomery forms 1 and l - 1, z = 0, x = 0, w = 0,
challenges that are their own inverse, w_O,i - y^i = 0, l_1,i = 0, a sum that lands exactly on l, <a_lo, b_hi> = 0, t_1 = 0, and witnesses of 0, 1, l - 1 and
2^252.  No tolerance anywhere: proof bytes and the transcript state after are compared with O.prove(..., script=), decisions with O.verify(..., script=).
No case is skipped or sampled; the parametrisation is by group and size with the cases looped inside, and a failure names the case.

Not reached here (they need n above 65,536 or 262,144, and stay with the 2^16 .. 2^20 fixtures under hashed challenges): the grid-stride loops of k_poly_t,
k_bt_poly_t, k_ipa_prep and k_verify_scalars, and the parts > 256 loop of k_reduce_partials."""
import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import script_cases as S

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 4
SCHEDULES = {"fold_group_1": {"BPG_TT_LG": 0, "BPG_FOLD_GROUP": 1}, "fold_group_3": {"BPG_TT_LG": 0, "BPG_FOLD_GROUP": 3},
             "tail_of_8_folded": {"BPG_TT_LG": 3, "BPG_TT_ORIG_LG": 0, "BPG_FOLD_GROUP": 2}}
SUBSETS = {"one-N8": lambda c: c.group == "one" and c.circuit.N == 8, "one-N64": lambda c: c.group == "one" and c.circuit.N == 64,
           "all-small": lambda c: c.group == "all" and c.circuit.N <= 64, "all-N512": lambda c: c.group == "all" and c.circuit.N == 512,
           "all-N1024": lambda c: c.group == "all" and c.circuit.N == 1024, "cancel-N64": lambda c: c.group == "cancel" and c.circuit.N == 64,
           "cancel-N1024": lambda c: c.group == "cancel" and c.circuit.N == 1024, "witness": lambda c: c.group == "witness"}


def subset(key):
    cases = [c for c in S.catalogue() if SUBSETS[key](c)]
    assert cases
    return cases


def test_subsets_cover_the_catalogue():
    assert sorted(c.name for k in SUBSETS for c in subset(k)) == sorted(c.name for c in S.catalogue())


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(S.GENS_CAPACITY)
    yield c
    c.close()


@pytest.fixture
def make_ctx(monkeypatch):
    """A fresh context with the given environment knobs (they are read once, at context creation)."""
    made = []

    def make(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        c = bpg.Context(0)
        made.append(c)
        for k in env:
            monkeypatch.delenv(k)
        c.gens_ensure(S.GENS_CAPACITY)
        return c
    yield make
    for c in made:
        c.close()


def vb_of(case):
    return b"".join(S.le(x) for x in case.circuit.vb)


def prove_single(c, case):
    rc = c.upload(case.circuit.inst)
    try:
        return rc.test_prove_scripted(case.circuit.state, vb_of(case), S.script_bytes(case.script), case.seed, case.flags)
    finally:
        rc.free()


_single = {}


def single(c, case):
    """the scripted single prover on the default schedule, once per case"""
    if case.name not in _single:
        _single[case.name] = prove_single(c, case)
    return _single[case.name]


def check_proof(case, got, what):
    want = S.reference(case.name)
    assert got[0] == want[0], "%s, %s: the proof differs from the scripted oracle's (first byte %d of %d)" % (
        case.name, what, next(i for i, (a, b) in enumerate(zip(got[0] + b"\0", want[0] + b"\1")) if a != b), len(want[0]))
    assert got[1] == want[1], "%s, %s: the transcript state after differs" % (case.name, what)


# ---------------------------------------------------------------------------------------------------- the scalar operations themselves
def test_device_scalar_add_sub_neg_and_words_at_their_edges(ctx):
    """sc_add, sc_sub, sc_neg and sc_to_words as the DEVICE compiles them (k_test_fe, ops 7 .. 10), raw words out, against Python integers: operands at 0, 1,
    l - 1, 2^252, equal operands, a + b = l exactly.  Inside a proof a result of l in place of 0 never shows - whatever consumes it (sc_add, sc_mont_mul,
    sc_to_words) reduces it - so no whole-proof test can pin that these return CANONICAL values; this one does."""
    L = S.L
    edge = [0, 1, 2, L - 1, L - 2, (L + 1) // 2, (L - 1) // 2, 2**252, 2**252 - 1, 2**252 + 1, 2**128, 2**32 - 1, 2**32, 2**64 - 1, 2**224, S.R_INV, L - S.R_INV]
    vals = edge + [S.filler(b"sc edge", i) for i in range(100)]
    pairs = [(a, b) for a in edge for b in edge] + [(a, a) for a in vals] + [(a, L - a) for a in vals if a] + list(zip(vals, vals[1:] + vals[:1]))
    assert any(a == b for a, b in pairs) and any(a and a + b == L for a, b in pairs) and (0, 0) in pairs
    A, B = [S.le(a) for a, _ in pairs], [S.le(b) for _, b in pairs]
    rinv = pow(2, -256, L)
    for op, f in ((7, lambda a, b: (a + b) % L), (8, lambda a, b: (a - b) % L), (9, lambda a, b: (-a) % L), (10, lambda a, b: a * rinv % L)):
        for (a, b), got in zip(pairs, ctx.test_fe_ops(op, A, B)):
            assert int.from_bytes(got, "little") == f(a, b), "op %d on %x, %x" % (op, a, b)


# ---------------------------------------------------------------------------------------------------- the single prover
@pytest.mark.parametrize("key", list(SUBSETS))
def test_single_prover_default_schedule(ctx, key):
    for case in subset(key):
        check_proof(case, single(ctx, case), "single prover")


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_single_prover_other_schedules(make_ctx, schedule, N):
    """the schedules without a table-driven tail from the start: k_ipa_prep, the MSM and the generator folds get challenges of 1, 2 and l - 1 and the cancellations"""
    c = make_ctx(**SCHEDULES[schedule])
    cases = [x for x in S.catalogue() if x.group in ("all", "cancel") and x.circuit.N == N]
    assert len(cases) == 5 + 6
    for case in cases:
        check_proof(case, prove_single(c, case), schedule)


# ---------------------------------------------------------------------------------------------------- the lockstep wave
def lockstep_list():
    """every one-position case, the witness edges, the N = 64 cancellations and the small all-at-once cases: lg N = 0, 1, 3 and 6, so that four groups of waves form,
    the lg N = 1 group holding ONE item (a wave of K = 1 inside the call)"""
    keep = lambda c: (c.group in ("one", "witness") or (c.group == "cancel" and c.circuit.N == 64) or (c.group == "all" and c.circuit.N in (1, 8) and c.circuit.n)
                      or c.name == "all/N2/l-1/flags3")
    out = [c for c in S.catalogue() if keep(c)]
    assert sorted({c.circuit.lgN for c in out}) == [0, 1, 3, 6] and sum(c.circuit.lgN == 1 for c in out) == 1
    assert {c.flags for c in out} == {0, 3}
    return out


def prove_lockstep(c, cases):
    got = c.test_prove_batch_scripted([(x.circuit.inst, x.circuit.state, vb_of(x), x.seed, x.flags) for x in cases], [S.script_bytes(x.script) for x in cases])
    assert len(got) == len(cases)
    return got


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_lockstep_wave_in_one_call(ctx, order):
    """ONE prove_batch call for the whole list; reversed, every edge sits at another item index of its wave"""
    cases = lockstep_list()
    if order == "reversed":
        cases = cases[::-1]
    for case, got in zip(cases, prove_lockstep(ctx, cases)):
        check_proof(case, got, "lockstep item of %d, %s" % (len(cases), order))
        assert got == single(ctx, case), "%s: the lockstep wave and the single prover differ" % case.name


def test_lockstep_wave_of_one(ctx):
    for name in ("one/N8/x=0", "one/N64/u_6=l-1", "witness/N64/all=l-1", "all/N1/1/flags0"):
        case = S.by_name(name)
        check_proof(case, prove_lockstep(ctx, [case])[0], "lockstep, K = 1")


def test_lockstep_small_waves(make_ctx):
    """the same items cut into many small waves: the ping-pong halves and the per-item offsets at other wave sizes"""
    c = make_ctx(BPG_BATCH_WAVE_MB=1)
    cases = [x for x in lockstep_list() if x.circuit.N == 64]
    for case, got in zip(cases, prove_lockstep(c, cases)):
        check_proof(case, got, "lockstep, waves of at most 1 MB")


# ---------------------------------------------------------------------------------------------------- the verifiers
def verifier_instance(case):
    return case.circuit.instance(witness=False)


def verify_single(c, case, proof, script=None):
    rc = c.upload(verifier_instance(case))
    try:
        return rc.test_verify_scripted(case.circuit.state, case.circuit.V, proof, S.script_bytes(case.script if script is None else script), S.SEED, case.flags)
    finally:
        rc.free()


@pytest.mark.parametrize("key", list(SUBSETS))
def test_verifier_decides_as_the_oracle_on_honest_proofs(ctx, key):
    for case in subset(key):
        proof, after = S.reference(case.name)
        want = S.oracle_verify(case, proof)
        assert want == (0 if S.case_satisfied(case.name) else O.ERR_VERIFY)
        status, state = verify_single(ctx, case, proof)
        assert status == want, case.name
        assert state == after, case.name


def rejected_and_hidden():
    """[(name, case, proof, script, the oracle's decision)]: the pinned tampers, and proofs under a script with another y"""
    out = [(name, case, proof, case.script, S.oracle_verify(case, proof)) for name, case, proof in S.tampers()]
    for name in ("one/N8/y=2", "one/N64/z=0", "cancel/N64/x=0", "all/N1024/2/flags3", "all/N1/2/flags0"):
        case = S.by_name(name)
        other = S.wrong_script(case)
        out.append((name + "#other y", case, S.reference(name)[0], other, S.oracle_verify(case, S.reference(name)[0], other)))
    assert {r[4] for r in out} == {0, O.ERR_VERIFY}                                        # x = 0 hides a tampered T_1; at N = 1 no y matters
    return out


def test_verifier_decides_as_the_oracle_on_tampered_proofs_and_other_scripts(ctx):
    for name, case, proof, script, want in rejected_and_hidden():
        assert verify_single(ctx, case, proof, script)[0] == want, name


def verify_batch(c, records, batch_seed=bytes(range(32, 64))):
    """records = [(case, proof, script)] -> statuses"""
    rc, statuses, _ = c.test_verify_batch_scripted([(verifier_instance(case), case.circuit.state, case.circuit.V, proof, S.SEED, case.flags) for case, proof, _ in records],
                                                   [S.script_bytes(script) for _, _, script in records], batch_seed)
    assert rc == next((s for s in statuses if s), 0)
    return statuses


def test_verify_batch_accepts_every_honest_small_proof_in_one_call(ctx):
    cases = [c for c in S.catalogue() if S.case_satisfied(c.name) and c.circuit.N <= 64]
    assert len(cases) > 150
    assert verify_batch(ctx, [(c, S.reference(c.name)[0], c.script) for c in cases]) == [0] * len(cases)


def test_verify_batch_with_accepted_and_rejected_items_in_one_call(ctx):
    records, want = [], []
    honest = [S.by_name(n) for n in ("one/N8/x=0", "one/N8/w=0", "one/N64/y=l-1", "all/N1n0/2/flags3", "cancel/N1024/cL=0", "witness/N8/all=1", "all/N512/l-1/flags0")]
    for k, (name, case, proof, script, decision) in enumerate(rejected_and_hidden()):
        if k % 6 == 0:                                                                      # honest proofs between the others
            h = honest[(k // 6) % len(honest)]
            records.append((h, S.reference(h.name)[0], h.script)); want.append(S.oracle_verify(h, S.reference(h.name)[0]))
        records.append((case, proof, script)); want.append(decision)
    assert want.count(0) > 5 and want.count(O.ERR_VERIFY) > 20
    assert verify_batch(ctx, records) == want


# ---------------------------------------------------------------------------------------------------- refusals, before any launch
def test_hooks_refuse_bad_scripts_and_items_off_the_lockstep_path(ctx):
    case, n0 = S.by_name("one/N8/y=2"), S.by_name("all/N1n0/2/flags0")
    good, proof = S.script_bytes(case.script), S.reference(case.name)[0]
    item = (case.circuit.inst, case.circuit.state, vb_of(case), case.seed, 0)
    vitem = (verifier_instance(case), case.circuit.state, case.circuit.V, proof, S.SEED, 0)
    bad = [good[:-1], good + [S.le(1)], [S.le(S.L)] + good[1:], good[:6] + [b"\xff" * 32] + good[7:], [bytes(32)] + good[1:], good[:5] + [bytes(32)] + good[6:], good[:7] + [bytes(32)]]
    rc = ctx.upload(case.circuit.inst)
    try:
        for script in bad:
            for call in (lambda: rc.test_prove_scripted(case.circuit.state, vb_of(case), script, case.seed, 0),
                         lambda: rc.test_verify_scripted(case.circuit.state, case.circuit.V, proof, script, S.SEED, 0),
                         lambda: ctx.test_prove_batch_scripted([item, item], [good, script]),
                         lambda: ctx.test_verify_batch_scripted([vitem, vitem], [good, script])):
                with pytest.raises(bpg.BpgError) as e:
                    call()
                assert e.value.status == INVALID_ARGUMENT and "scripted:" in str(e.value)
    finally:
        rc.free()
    with pytest.raises(bpg.BpgError) as e:                                                  # n = 0 takes the single path in bpg_r1cs_prove_batch
        ctx.test_prove_batch_scripted([item, (n0.circuit.inst, n0.circuit.state, vb_of(n0), n0.seed, 0)], [good, S.script_bytes(n0.script)])
    assert e.value.status == INVALID_ARGUMENT and "not lockstep-eligible" in str(e.value)
