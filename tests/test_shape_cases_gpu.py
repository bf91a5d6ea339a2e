"""Every case of the shape catalogue (tests/shape_cases.py) through every upload path of the product - the single upload, the lockstep wave of prove_batch,
templates with assign, template batches, device-made repeats and joins, batch verification, check() - byte for byte against the CPU oracle, and the
flattened weights (bpg_test_weights: the verifier's own k_flatten / k_flatten_const path) against the integer model.  No tolerance, no timing, no case
skipped.  What the catalogue holds and why is in shape_cases.py; test_shape_cases_host.py pins it without a device.

The lockstep tests are the ones a wave of TALL items (more rows than 3 K N + mT) used to break: the transposition's second scan takes `counts` as scratch
for qT words, and the wave laid `counts` out for its columns only (csrc/host/csc_work.hpp now sizes it in one place, for upload() and the wave alike).

A template needs a witness program; the catalogue's rows cannot come out of a Prover's gadget calls (multiply() adds its own two rows), so a case becomes a
template through Context.upload_template - which is all Prover.template() calls - under a program of constants (shape_cases.template_parts): the rows are
the case's own, entry for entry.  Repeats and joins are proved where the result fits the shared context's 1024 generators; their weights are checked always."""
import ctypes as C

import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import script_cases as S
import shape_cases as H

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 4
NAMES = H.names()
LOCKSTEP = [c.name for c in H.lockstep_cases()]


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(H.GENS_CAPACITY)
    yield c
    c.close()


def flags_of(k):
    return 3 if k % 2 else 0


_single = {}


def single(ctx, case, k=0, flags=0):
    """upload + prove of the case alone under seed k, once"""
    key = (case.name, k, flags)
    if key not in _single:
        c = case.circuit
        rc = ctx.upload(c.inst)
        try:
            _single[key] = rc.prove(c.state, H.vb_of(c), H.seed(k), flags)
        finally:
            rc.free()
    return _single[key]


def same(got, want, what):
    assert got[0] == want[0], "%s: the proof differs from the oracle's (first byte %d of %d)" % (
        what, next(i for i, (a, b) in enumerate(zip(got[0] + b"\0", want[0] + b"\1")) if a != b), len(want[0]))
    assert got[1] == want[1], "%s: the transcript state after differs" % what


def verifier_upload(ctx, circ, rows=None):
    return ctx.upload(circ.instance(rows, witness=False))


# ---------------------------------------------------------------------------------------------------- the single path
@pytest.mark.parametrize("name", NAMES)
def test_single_upload_prove_verify_and_one_tamper(ctx, name):
    case = H.by_name(name)
    c = case.circuit
    for flags in (0, 3):
        same(single(ctx, case, 0, flags), H.reference(name, 0, flags), "%s, flags %d" % (name, flags))
    proof = single(ctx, case)[0]
    assert H.oracle_verify(c, proof) == 0
    rc = verifier_upload(ctx, c)
    try:
        assert rc.verify(c.state, c.V, proof, S.SEED, 0) == 0
    finally:
        rc.free()
    rows = H.tampered_rows(c)
    assert (rows is None) == (H.nnz_of(c) == 0)
    if rows is not None:                    # one constant (or coefficient) of the last non-empty row: w_c (or one weight) on this shape
        want = H.oracle_verify(c, proof, 0, rows)
        assert want == O.ERR_VERIFY
        rc = verifier_upload(ctx, c, rows)
        try:
            assert rc.verify(c.state, c.V, proof, S.SEED, 0) == want
        finally:
            rc.free()


@pytest.mark.parametrize("name", NAMES)
def test_weights_equal_the_model(ctx, name):
    c = H.by_name(name).circuit
    rc = verifier_upload(ctx, c)
    try:
        for zname, z in H.Z_VALUES:
            assert rc.test_weights(H.le(z)) == H.model_bytes(c, z), "%s at z = %s" % (name, zname)
    finally:
        rc.free()


@pytest.mark.parametrize("name", NAMES)
def test_check_names_the_broken_row(ctx, name):
    """check() finds the case satisfied; with the witness made to miss ONE row - row 0, row q - 1, the row right behind the run of empty rows - it names that row
    and no other.  A witness value sits in many rows, so the row is broken from its own side (shape_cases.break_row: its constant, or a coefficient, plus one):
    to check() that is the same witness against a row it no longer satisfies.  An empty row cannot be missed and is left out (pinned in the test below)"""
    case = H.by_name(name)
    c = case.circuit
    assert ctx.check_flat(c.inst).ok
    for r in H.rows_to_break(case):
        rep = ctx.check_flat(c.instance(H.break_row(c, r)))
        assert (rep.bad_multipliers, rep.bad_rows, rep.first_bad_row, rep.rows) == (0, 1, r, [r]), (name, r, rep)


def test_rows_to_break_cover_the_ends_and_the_row_after_a_run():
    got = {c.name: H.rows_to_break(c) for c in H.catalogue()}
    assert got["empty/run300"] == [0, 500, 529] and got["empty/first"] == [1, 5] and got["empty/last"] == [0] and got["empty/all"] == []
    assert got["tall/n1-m1-q2100"] == [0, 2099] and got["wide/q1-n700"] == [0] and got["wide/q0-n5"] == []


# ---------------------------------------------------------------------------------------------------- the lockstep wave
def test_lockstep_takes_every_case_with_a_multiplier():
    assert sorted(set(NAMES) - set(LOCKSTEP)) == sorted(c.name for c in H.catalogue() if c.circuit.n == 0) == ["tall/n0-m2-q300"]


def item_of(case, k, flags):
    c = case.circuit
    return (c.inst, c.state, H.vb_of(c), H.seed(k), flags)


def prove_batch_logged(ctx, items):
    """prove_batch under the launch log (profile mode 2) -> (results, {kernel: launches})"""
    ctx.profile_set(2)
    try:
        res = ctx.prove_batch(items)
        counts = {k: v["count"] for k, v in ctx.profile_report().items() if v["count"]}
    finally:
        ctx.profile_set(0)
    return res, counts


def check_wave_log(counts, waves, waves_with_rows, what):
    """the k_bt_* wave ran - once per wave - and the matrix was transposed once per wave, not once per item"""
    assert counts.get("k_bt_commit3") == waves and counts.get("k_bt_exp") == waves, (what, counts)
    assert counts.get("k_csc_colptr") == waves and counts.get("k_csc_fill", 0) == waves_with_rows and counts.get("k_csc_count", 0) == waves_with_rows, (what, counts)
    assert "k_poly_t" not in counts and "k_tt_commit3" not in counts, (what, counts)            # nothing took the single prover


@pytest.mark.parametrize("name", LOCKSTEP)
def test_lockstep_wave_of_one_shape(ctx, name):
    """K = 8 copies of the case under eight seeds, the dialects 0 and 3 alternating: one wave"""
    case = H.by_name(name)
    items = [item_of(case, k, flags_of(k)) for k in range(H.LOCKSTEP_K)]
    res, counts = prove_batch_logged(ctx, items)
    for k, got in enumerate(res):
        same(got, H.reference(name, k, flags_of(k)), "%s, item %d of the wave" % (name, k))
        assert got == single(ctx, case, k, flags_of(k)), "%s, item %d: the wave and the single prover differ" % (name, k)
    check_wave_log(counts, 1, 1 if H.q_of(case.circuit) else 0, name)


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_lockstep_mixed_wave(ctx, order):
    """ONE call holds every eligible case once: a wave per padded size, each a block-diagonal matrix of different shapes; reversed, every shape sits at another
    item index and row base of its wave"""
    cases = H.lockstep_cases()
    if order == "reversed":
        cases = cases[::-1]
    res, counts = prove_batch_logged(ctx, [item_of(c, 0, 0) for c in cases])
    for case, got in zip(cases, res):
        same(got, H.reference(case.name), "%s in the mixed call, %s" % (case.name, order))
        assert got == single(ctx, case), case.name
    rows_by_N = {}
    for c in cases:
        rows_by_N[c.circuit.N] = rows_by_N.get(c.circuit.N, 0) + H.q_of(c.circuit)
    assert len(rows_by_N) >= 4
    check_wave_log(counts, len(rows_by_N), sum(1 for q in rows_by_N.values() if q), order)


# ---------------------------------------------------------------------------------------------------- templates
def template_of(ctx, circ):
    inst, prog = H.template_parts(circ)
    return ctx.upload_template(inst, prog), inst, prog


@pytest.mark.parametrize("name", LOCKSTEP)
def test_template_assign_prove(ctx, name):
    c = H.by_name(name).circuit
    t, _, _ = template_of(ctx, c)
    try:
        t.assign(H.v_of(c))
        assert t.check().ok
        same(t.prove(c.state, H.vb_of(c), H.seed(0), 0), H.reference(name), name + " as a template")
        assert t.test_weights(H.le(H.Z_VALUES[3][1])) == H.model_bytes(c, H.Z_VALUES[3][1])
    finally:
        t.free()


TEMPLATE_BATCH = [n for n in LOCKSTEP if n.startswith(("tall/", "hot/"))]


@pytest.mark.parametrize("name", TEMPLATE_BATCH)
def test_template_batch(ctx, name):
    """prove_template_batch, K = 8: the template's rows repeated down the wave's block-diagonal matrix"""
    assert len(TEMPLATE_BATCH) == 5
    c = H.by_name(name).circuit
    t, _, _ = template_of(ctx, c)
    try:
        res = t.prove_batch([(H.v_of(c), b"", c.state, H.vb_of(c), H.seed(k), flags_of(k)) for k in range(H.LOCKSTEP_K)])
        for k, got in enumerate(res):
            same(got, H.reference(name, k, flags_of(k)), "%s, item %d of the template batch" % (name, k))
    finally:
        t.free()


def prove_assembled(asm, k=0):
    rc, proof, after = O.prove(H.gens(), asm.state, S.oracle_circuit(asm), H.vb_of(asm), H.seed(k), O.FLAG_FAST_MSM)
    assert rc == 0
    return proof, after


def check_composite(res, asm, what):
    """a device-made repeat or join against the host-assembled circuit it stands for: the weights always, the proof where the generators reach"""
    assert (res.n, res.m) == (asm.n, asm.m)
    for zname, z in H.Z_VALUES:
        assert res.test_weights(H.le(z)) == H.model_bytes(asm, z), "%s at z = %s" % (what, zname)
    if asm.N > H.GENS_CAPACITY:
        return False
    res.assign(H.v_of(asm))
    assert res.check().ok
    same(res.prove(asm.state, H.vb_of(asm), H.seed(0), 0), prove_assembled(asm), what)
    return True


REPEATED = [n for n in LOCKSTEP if n.startswith(("tall/", "wide/", "sect/"))]


@pytest.mark.parametrize("name", REPEATED)
def test_template_repeat(ctx, name):
    assert len(REPEATED) == 3 + 3 + 4
    c = H.by_name(name).circuit
    t, inst, prog = template_of(ctx, c)
    rep = t.repeat(3)
    try:
        asm = H.assembled(name + " x3", c.label, [(c, 3)], bpg.test_template_repeat_instance(inst, prog, None, 3))
        assert S.satisfied(asm) and H.q_of(asm) == 3 * H.q_of(c)
        proved = check_composite(rep, asm, name + " repeated")
        assert proved == (name != "wide/q1-n700")          # 2100 multipliers: beyond the shared context's generators, weights only
    finally:
        rep.free(); t.free()


@pytest.mark.parametrize("pair", [("tall/n3-m2-q600", "wide/q0-n2-m3"), ("wide/q0-n5", "tall/n1-m1-q2100"), ("const/none", "const/all")])
def test_template_join(ctx, pair):
    a, b = (H.by_name(n).circuit for n in pair)
    ta, ia, pa = template_of(ctx, a)
    tb, ib, pb = template_of(ctx, b)
    joined = ctx.join([(ta, 1), (tb, 2)])
    try:
        asm = H.assembled(" + ".join(pair), a.label, [(a, 1), (b, 2)], bpg.test_template_join_instance([(ia, pa, None, 1), (ib, pb, None, 2)]))
        assert S.satisfied(asm) and H.q_of(asm) == H.q_of(a) + 2 * H.q_of(b)
        assert check_composite(joined, asm, "join of %s and 2 x %s" % pair)
    finally:
        joined.free(); ta.free(); tb.free()


# ---------------------------------------------------------------------------------------------------- batch verification
def test_verify_batch_names_the_one_tampered_item(ctx):
    """every single-path proof in ONE verify_batch call, one of them with t_x + 1: the batch rejects and names exactly that item"""
    cases = list(H.catalogue())
    proofs = [single(ctx, c)[0] for c in cases]
    bad = NAMES.index("tall/n3-m2-q600")
    at = 192 + 160
    proofs[bad] = proofs[bad][:at] + H.le((int.from_bytes(proofs[bad][at:at + 32], "little") + 1) % H.L) + proofs[bad][at + 32:]
    assert H.oracle_verify(cases[bad].circuit, proofs[bad]) == O.ERR_VERIFY
    items = [(c.circuit.instance(witness=False), c.circuit.state, c.circuit.V, p, S.SEED, 0) for c, p in zip(cases, proofs)]
    rc, statuses, _ = ctx.verify_batch(items, batch_seed=bytes(range(32, 64)), return_status=True)
    assert statuses == [O.ERR_VERIFY if k == bad else 0 for k in range(len(cases))] and rc == O.ERR_VERIFY
    rc, statuses, states = ctx.verify_batch(items[:bad] + items[bad + 1:], batch_seed=bytes(range(32, 64)), return_status=True)
    assert rc == 0 and statuses == [0] * (len(cases) - 1)
    assert states == [single(ctx, c)[1] for c in cases[:bad] + cases[bad + 1:]]


# ---------------------------------------------------------------------------------------------------- the hook's refusals, before any launch
def test_weights_hook_refusals(ctx):
    c = H.by_name("edge/n7").circuit
    rc = verifier_upload(ctx, c)
    try:
        for z in (None, H.le(H.L), b"\xff" * 32):
            with pytest.raises(bpg.BpgError) as e:
                rc.test_weights(z)
            assert e.value.status == INVALID_ARGUMENT
        out = C.create_string_buffer(b"\x5a" * 32 * (3 * c.n + c.m + 1), 32 * (3 * c.n + c.m + 1))
        lib = bpg.lib()
        assert lib.bpg_test_weights(ctx._h, rc._h, H.le(H.L), out) == INVALID_ARGUMENT and b"canonical" in lib.bpg_last_error()
        assert lib.bpg_test_weights(ctx._h, None, H.le(1), out) == INVALID_ARGUMENT
        assert lib.bpg_test_weights(ctx._h, rc._h, H.le(1), None) == INVALID_ARGUMENT
        assert out.raw == b"\x5a" * len(out.raw)
        assert rc.test_weights(H.le(1)) == H.model_bytes(c, 1)
    finally:
        rc.free()
