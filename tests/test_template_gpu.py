"""Circuit templates on the GPU: a template that was assigned a fresh witness proves exactly what the existing path - host assembly of that witness,
bpg_r1cs_upload, bpg_r1cs_prove_resident - proves, byte for byte, with the same transcript state, blindings and rng seed; and the CPU oracle's verifier
accepts the proof.  The host assembly (and through it the oracle) is the yardstick everywhere; the template path is never compared with itself."""
import hashlib
import os

import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O

pytestmark = pytest.mark.gpu
L = bpg.L
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    yield c
    c.close()


def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


def constant_term(inst, row):
    """the constant term of a constraint row of a host-assembled instance (sum of its One terms): what assign() is given for a parameter row"""
    a, b = int(inst.row_ptr[row]), int(inst.row_ptr[row + 1])
    s = sum(int.from_bytes(inst.coef[32 * int(inst.term_coef[k]):32 * int(inst.term_coef[k]) + 32], "little") for k in range(a, b) if int(inst.term_var[k]) >> 29 == 4)
    return (s % L).to_bytes(32, "little")


def last_row(a):
    return a.prover.num_constraints() - 1


def host_proof(ctx, a, seed=SEED):
    """the existing path: the host-assembled instance, uploaded and proved"""
    inst = a.prover.instance()
    res = ctx.upload(inst)
    proof, _ = res.prove(a.transcript.state, inst.v_blinding, seed)
    res.free()
    return inst, proof


def assign_and_prove(tmpl, a, inst, seed=SEED):
    tmpl.assign(inst.v, [constant_term(inst, last_row(a))])
    proof, _ = tmpl.prove(a.transcript.state, inst.v_blinding, seed)
    return proof


def oracle_accepts(ogens, a, inst, proof):
    return O.verify(ogens, a.transcript.state, to_oracle(inst), b"".join(a.commitments), proof) == 0


@pytest.mark.parametrize("leaves", [8, 64])
def test_merkle_witness_equality(ctx, leaves):
    base = workloads.merkle_full_tree(ctx, leaves=leaves, seed=1)
    ctx.gens_ensure(base.gens_capacity)
    ogens = O.Gens(base.gens_capacity)
    tmpl = base.prover.template(ctx, param_rows=[last_row(base)])
    inst1, want1 = host_proof(ctx, base)
    assert tmpl.prove(base.transcript.state, inst1.v_blinding, SEED)[0] == want1          # the uploaded witness: no assign needed for the first proof
    for seed in (2, 3, 4, 5):
        a = workloads.merkle_full_tree(ctx, leaves=leaves, seed=seed)
        inst, want = host_proof(ctx, a)
        assert inst.v != inst1.v and a.root != base.root
        got = assign_and_prove(tmpl, a, inst)
        assert got == want, "seed %d: the assigned template and the host assembly give different proofs" % seed
        assert oracle_accepts(ogens, a, inst, got)
    tmpl.free()


def test_mimc_preimage_witness_equality(ctx):
    """cfg 3 (2^16) with the image as the parameter; 67 absorbed blocks = 67 levels of one segment"""
    base = workloads.mimc_preimage(ctx, seed=1)
    ctx.gens_ensure(base.gens_capacity)
    ogens = O.Gens(base.gens_capacity)
    tmpl = base.prover.template(ctx, param_rows=[last_row(base)])
    inst1, want1 = host_proof(ctx, base)
    assert tmpl.prove(base.transcript.state, inst1.v_blinding, SEED)[0] == want1          # the uploaded witness of seed 1
    for seed in (2, 3, 4, 5):
        a = workloads.mimc_preimage(ctx, seed=seed)
        inst, want = host_proof(ctx, a)
        assert inst.v != inst1.v
        got = assign_and_prove(tmpl, a, inst)
        assert got == want, "seed %d: the assigned template and the host assembly give different proofs" % seed
        assert oracle_accepts(ogens, a, inst, got)
    tmpl.free()


def test_template_without_a_witness_and_wrong_parameter(ctx):
    """A template uploaded WITHOUT a witness refuses to prove until assigned; a wrong parameter (the root of another seed) is really patched into the
    constraint: the proof - which does not depend on constants - is rejected by the GPU verifier on the template, and accepted with the right root."""
    a, b = workloads.merkle_full_tree(ctx, leaves=8, seed=2), workloads.merkle_full_tree(ctx, leaves=8, seed=3)
    ctx.gens_ensure(a.gens_capacity)
    inst, instb = a.prover.instance(), b.prover.instance()
    prog = a.prover.witness_program(); prog.param_rows = [last_row(a)]
    import ctypes as C
    cs, cp, h = inst.cstruct(), prog.cstruct(), C.c_void_p()
    cs.aL = cs.aR = cs.aO = None
    assert bpg.lib().bpg_r1cs_upload_template(ctx._h, C.byref(cs), C.byref(cp), C.byref(h)) == 0, bpg.lib().bpg_last_error()
    tmpl = bpg.ResidentCircuit(ctx, h, inst.n, inst.m, n_params=1)
    with pytest.raises(bpg.BpgError) as e:
        tmpl.prove(a.transcript.state, inst.v_blinding, SEED)
    assert e.value.status == 5
    _, want = host_proof(ctx, a)
    coms = b"".join(a.commitments)
    tmpl.assign(inst.v, [constant_term(instb, last_row(b))])                        # the root of seed 3 under the leaves of seed 2
    proof, _ = tmpl.prove(a.transcript.state, inst.v_blinding, SEED)
    assert proof == want
    assert tmpl.verify(a.transcript.state, coms, proof) == 3                        # BPG_ERR_VERIFICATION
    tmpl.assign(inst.v, [constant_term(inst, last_row(a))])
    assert tmpl.verify(a.transcript.state, coms, proof) == 0
    assert ctx.verify_flat(inst, a.transcript.state, coms, proof) == 0
    # argument checks on a live handle
    plain = ctx.upload(inst)
    for c, vals, params in ((plain, inst.v, []), (tmpl, inst.v, []), (tmpl, inst.v[32:], [bytes(32)]), (tmpl, inst.v, [bytes(32)] * 2)):
        with pytest.raises((bpg.BpgError, ValueError)) as e:
            c.assign(vals, params)
        assert not isinstance(e.value, bpg.BpgError) or e.value.status == 4
    plain.free(); tmpl.free()


def test_unreduced_committed_value(ctx):
    """committed values with the top bits set (Scalar::from_bits admits anything below 2^255): the host assembly's witness"""
    def tree(leaf_ints):
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        leaves = [x.to_bytes(32, "little") for x in leaf_ints]
        coms, vs = p.commit_many(leaves, [workloads.blinding("unred", i) for i in range(len(leaves))])
        probe = bpg.Prover(None, bpg.Transcript(b"probe"))
        bpg.MerkleTree256(bytes(32), leaves, [], "((I I) (I I))").prove(probe, [], [])
        bpg.MerkleTree256(probe.instance().aO[-32:], [], bpg.vars_to_lc(vs), "((W W) (W W))").prove(p, [], [])
        return workloads.Assembled(p, t, coms, 8192, None), b"".join(leaves)
    ctx.gens_ensure(8192)
    base, _ = tree([11, 12, 13, 14])
    a, raw = tree([(1 << 254) | (L + 5), (1 << 255) - 19, L, 3 * L + 7])
    assert all(int.from_bytes(raw[i:i + 32], "little") >= L for i in range(0, 128, 32))
    tmpl = base.prover.template(ctx, param_rows=[last_row(base)])
    inst, want = host_proof(ctx, a)
    tmpl.assign(raw, [constant_term(inst, last_row(a))])                            # the unreduced bytes, as handed to commit()
    assert tmpl.prove(a.transcript.state, inst.v_blinding, SEED)[0] == want
    assert oracle_accepts(O.Gens(8192), a, inst, want)
    tmpl.free()


def test_merge_sets_are_rebuilt_for_every_witness(monkeypatch):
    """BPG_MERGE=1 groups equal scalars of a_L, a_R, a_O once per resident witness, at its first proof.  assign() must drop the groups of the previous
    witness: a stale set gives a wrong A_I without any error.  (Checked once with the invalidation taken out of Engine::assign: this test then fails:
    the first proof after an assign differs.)  64 leaves: N = 2^17, above the table-driven path that does not merge; an equal-leaves tree (groups of dozens of terms) is
    assigned after a distinct-leaves witness and back.  The reference's own 512-equal-leaves instance: test_full_size_merge_sequence."""
    monkeypatch.setenv("BPG_MERGE", "1")
    ctx = bpg.Context(0)
    a, b, eq = (workloads.merkle_full_tree(ctx, leaves=64, seed=s) for s in (2, 3, None))
    ctx.gens_ensure(a.gens_capacity)
    want = {k: host_proof(ctx, x) for k, x in (("a", a), ("b", b), ("eq", eq))}
    tmpl = a.prover.template(ctx, param_rows=[last_row(a)])
    assert tmpl.prove(a.transcript.state, want["a"][0].v_blinding, SEED)[0] == want["a"][1]      # builds the sets of witness a
    for k, x in (("b", b), ("eq", eq), ("a", a), ("eq", eq)):
        assert assign_and_prove(tmpl, x, want[k][0]) == want[k][1], "after assigning %s" % k
        assert tmpl.prove(x.transcript.state, want[k][0].v_blinding, SEED)[0] == want[k][1]       # ... and with the sets of this witness in place
    tmpl.free(); ctx.close()


def test_full_size_merge_sequence(monkeypatch):
    """2^20 under BPG_MERGE=1 on a context of its own (n = 993,384, 18 levels of at most 256 segments).  The template is made from a distinct-leaves tree
    and proved (its merge sets exist); then a fresh distinct seed is assigned, then the reference's 512-EQUAL-leaves instance (merkle_tree_gadget.rs:473-545:
    its merge sets are the largest there are - nearly every term of A_I and A_O is merged away), then a distinct witness again, and the reference's once
    more.  Every proof equals the one a fresh upload of that witness's host assembly gives, also when proved a second time with its own sets in place;
    the oracle's verifier accepts the fresh seed's proof (its prover would need minutes at this size)."""
    monkeypatch.setenv("BPG_MERGE", "1")
    ctx = bpg.Context(0)
    base = workloads.merkle_full_tree(ctx, leaves=512, seed=7)
    fresh = workloads.merkle_full_tree(ctx, leaves=512, seed=20261016)
    ref = workloads.merkle_full_tree(ctx, leaves=512, seed=None)
    ctx.gens_ensure(base.gens_capacity)
    want = {k: host_proof(ctx, x) for k, x in (("base", base), ("fresh", fresh), ("ref", ref))}
    assert want["fresh"][0].n == 993384 and ctx.schedule()["merge_equal"] == 1
    tmpl = base.prover.template(ctx, param_rows=[last_row(base)])
    assert tmpl.prove(base.transcript.state, want["base"][0].v_blinding, SEED)[0] == want["base"][1]     # the template's own witness: builds its sets
    for k, x in (("fresh", fresh), ("ref", ref), ("base", base), ("ref", ref), ("fresh", fresh)):
        got = assign_and_prove(tmpl, x, want[k][0])
        assert got == want[k][1], "after assigning %s" % k
        if k == "ref":
            assert ctx.schedule()["merged_skipped_last"] > 2_000_000                                      # the equal-leaves sets really are the large ones
            assert tmpl.prove(x.transcript.state, want[k][0].v_blinding, SEED)[0] == want[k][1]           # ... and again with those sets in place
    G, Hh = ctx.gens_export(0, base.gens_capacity)
    assert oracle_accepts(O.Gens(compressed=(G, Hh)), fresh, want["fresh"][0], want["fresh"][1])
    tmpl.free(); ctx.close()


def test_fifty_fresh_witnesses_on_one_context():
    """assign -> prove fifty times on one context on a 2^12-sized circuit (the 3-leaf tree `((W W) W)`: four absorbed blocks, n = 3,888, N = 4,096) with
    the blinding chain of proof k+1 started before proof k is proved.  Every proof equals the one made for its witness alone (host assembly, upload,
    prove); device memory is the same before and after."""
    import ctypes as C
    ctx = bpg.Context(0)
    ctx.gens_ensure(4096)
    # the HIP runtime the library itself runs on (already mapped into this process)
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))

    def device_free():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    def tree(seed):
        cfg = "fifty-%d" % seed
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        leaves = [b"\x03" + workloads.synth(cfg, i, 31) for i in range(3)]
        scalars, coms, vs = bpg.commit_all_single(p, leaves, [workloads.blinding(cfg, i) for i in range(3)])
        probe = bpg.Prover(None, bpg.Transcript(b"probe"))
        bpg.MerkleTree256(bytes(32), [bpg.be_to_scalar(x) for x in leaves], [], "((I I) I)").prove(probe, [], [])
        bpg.MerkleTree256(probe.instance().aO[-32:], [], bpg.vars_to_lc(vs), "((W W) W)").prove(p, [], [])
        return workloads.Assembled(p, t, coms, 4096, None)

    def rng(k):
        return hashlib.sha256(b"fifty-rng-%d" % k).digest()

    items = [tree(s) for s in range(53)]
    insts = [x.prover.instance() for x in items]
    assert insts[0].n == 3888
    alone = {}
    for k in range(1, 53):
        res = ctx.upload(insts[k]); alone[k] = res.prove(items[k].transcript.state, insts[k].v_blinding, rng(k))[0]; res.free()
    tmpl = items[0].prover.template(ctx, param_rows=[last_row(items[0])])

    def round_(k, ahead):
        tmpl.assign(insts[k].v, [constant_term(insts[k], last_row(items[k]))])
        if ahead:
            ctx.blinding_begin(items[k + 1].transcript.state, insts[k + 1].v_blinding, rng(k + 1), 4096)     # one proof ahead
        got, _ = tmpl.prove(items[k].transcript.state, insts[k].v_blinding, rng(k))
        assert got == alone[k], "proof %d" % k

    ctx.blinding_begin(items[1].transcript.state, insts[1].v_blinding, rng(1), 4096)
    round_(1, True); round_(2, True)                                                # warm: every buffer of the loop has its size
    free0 = device_free()
    for k in range(3, 53):
        round_(k, k < 52)
    assert device_free() == free0, "device memory moved over fifty assign + prove rounds"
    tmpl.free(); ctx.close()
