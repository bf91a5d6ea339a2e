"""Random circuit templates on the GPU: every template entry point - assign, the lockstep batches, checkpoints, public inputs, repeat, join, check - on seeded
random shapes (tests/random_templates.py) that no gadget draws: n of 1, 2, 3 and just above a power of two, m = 0, q = 0, several parameter rows per item,
hint runs over arbitrary linear combinations with sparse bits, zero coefficients, empty lists, dozens of schedule levels.

The yardstick is never the template path: it is the HOST-ASSEMBLED instance of the same witness through the existing ctx.upload(...).prove(...), with the same
transcript state, blindings and rng seed - proof bytes and transcript state after, byte for byte.  The proof bytes fingerprint the whole of a_L, a_R, a_O and
every non-constant matrix entry; the constants are covered by verify(...) == 0 on the resident circuit and by check().  The CPU oracle's verifier judges the
proofs of the smaller shapes, and the generator's model (Python integers) says which checkpoint a wrong value breaks first.

PINNED (chosen on the CPU from the host module's range; n, m, q, hinted multipliers, levels, segments):
    45: (1, 0, 0, 1, 1, 1)     118: (1, 3, 0, 1, 1, 1)    112: (2, 0, 3, 1, 2, 2)     38: (2, 3, 5, 0, 1, 1)      73: (3, 3, 6, 1, 3, 3)      35: (3, 1, 3, 2, 1, 1)
    31: (8, 5, 18, 0, 6, 6)    13: (17, 1, 12, 12, 7, 8)  18: (17, 0, 24, 8, 5, 6)     9: (33, 4, 47, 12, 12, 16)  22: (65, 0, 72, 32, 19, 28)  44: (200, 5, 231, 101, 42, 107)
PINNED_PUBLIC: the same for the family with public inputs (another family of shapes: the inputs join the pool the terms are drawn from).
Everything is at N <= 256 but the larger repeats and joins (N <= 1024).

Run as a script (`python tests/test_template_random_gpu.py leak`) the file runs one scenario of every family in a process of its own, frees everything and
prints the census of what the process still holds (bpg_test_live_resources)."""
import hashlib
import json
import pathlib
import subprocess
import sys

if __name__ == "__main__":
    _root = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "tests"), str(_root / "tests" / "golden")]

import ctypes as C

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import random_templates as RT
import template_inputs_cases as TC
from test_template_host import StubProver
from test_template_hints_host import schedule_hinted
from test_template_checkpoints_host import schedule_ck
from test_template_inputs_host import schedule_inputs

pytestmark = pytest.mark.gpu
PINNED = [45, 118, 112, 38, 73, 35, 31, 13, 18, 9, 22, 44]
PINNED_PUBLIC = [19, 146, 172, 36, 182, 45, 121, 10, 33, 17, 103, 6]
SMALL = [s for s in PINNED if RT.shape(s).n <= 3]
CAPACITY = 1024
MISMATCH, MISSING, INVALID = bpg.ERR_CHECKPOINT_MISMATCH, 5, 4
LABEL = b"RandomTemplate"
ORACLE_N = 64                   # the oracle's verifier judges the proofs of circuits up to this padded size


def rng(tag):
    return hashlib.sha256(("random template %s" % (tag,)).encode()).digest()


def state_before():
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(LABEL)
    bpg.Prover(None, t)
    return t.state


def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


class Host:
    """ONE prover on the device context, items appended by `build(prover)` -> [Item]: the host assembly, its commitments, and what the existing path proves"""
    def __init__(self, ctx, build, tag):
        self.ctx, self.tag = ctx, tag
        t = bpg.Transcript(LABEL)
        self.prover = bpg.Prover(ctx, t)
        self.items = build(self.prover)
        self.inst = self.prover.instance()
        self.state = t.state
        self.coms = b"".join(self.prover.commitment(i) for i in range(self.inst.m))
        self.params = [x for it in self.items for x in it.params]
        self.N = 1 << (self.inst.n - 1).bit_length()
        self._want = {}

    def proof(self, flags=0):
        """the existing path: the host-assembled instance, uploaded and proved -> (proof, transcript state after)"""
        if flags not in self._want:
            res = self.ctx.upload(self.inst)
            try:
                self._want[flags] = res.prove(self.state, self.inst.v_blinding, rng(self.tag), flags)
            finally:
                res.free()
        return self._want[flags]

    def prove_on(self, circuit, flags=0):
        return circuit.prove(self.state, self.inst.v_blinding, rng(self.tag), flags)

    def oracle_accepts(self, proof):
        return O.verify(O.Gens(self.N), self.state, to_oracle(self.inst), self.coms, proof) == 0

    def batch_item(self, commit=False, flags=0, pre=None):
        """(values, params, state, blindings, rng seed, flags) of a one-item host assembly as the template batches take it"""
        return (self.inst.v, self.params, pre if commit else self.state, self.inst.v_blinding, rng(self.tag), flags)

    def result(self, commit, flags=0):
        return self.proof(flags) + ((self.coms,) if commit else ())


class Hosts:
    """the one-item host assemblies of the module, made on demand and kept: (family, shape seed, value seed) -> Host"""
    def __init__(self, ctx):
        self.ctx, self.have, self.pre = ctx, {}, state_before()

    def __call__(self, seed, vs, public=False):
        key = (public, seed, vs)
        if key not in self.have:
            build = (lambda p: [RT.item(p, seed, vs, TC.Public(p, False))]) if public else (lambda p: [RT.item(p, seed, vs)])
            self.have[key] = Host(self.ctx, build, key)
        return self.have[key]


def stub(seed, public=False, vs=0):
    """the shape assembled alone without a device: (instance - with its input terms where public -, program, hints, Item)"""
    p = StubProver(None, bpg.Transcript(LABEL))
    it = RT.item(p, seed, vs, TC.Public(p, True) if public else None)
    prog, hints = p.witness_program(hints=True)
    return (p.template_instance()[0] if public else p.instance()), prog, hints, it


def upload(ctx, seed, checkpoints=(), public=False, witness=False):
    """the template of the shape from value seed 0, WITHOUT a witness unless asked -> (ResidentCircuit, Item, schedule levels)"""
    inst, prog, hints, it = stub(seed, public)
    ck_vars = it.checkpoints(checkpoints)[0]
    if public:
        levels = schedule_inputs((inst, prog, hints, it.inputs), len(it.inputs), ck_vars)["levels"]
    else:
        levels = schedule_ck(inst, prog, hints, ck_vars)["levels"] if ck_vars else schedule_hinted(inst, prog, hints)["levels"]
    if witness:
        return ctx.upload_template(inst, prog, hints, checkpoints=ck_vars or None, inputs=it.inputs if public else None), it, levels
    cs, cp, h = inst.cstruct(), prog.cstruct(), C.c_void_p()
    cs.aL = cs.aR = cs.aO = None
    ch = hints.cstruct() if len(hints) else None
    ck = bpg._checkpoints_cstruct(ck_vars)
    lib, hp = bpg.lib(), (C.byref(ch) if ch is not None else None)
    if public:
        st = lib.bpg_r1cs_upload_template_inputs(ctx._h, C.byref(cs), C.byref(cp), hp, C.byref(ck), C.c_uint64(len(it.inputs)), None, C.byref(h))
    elif ck_vars:
        st = lib.bpg_r1cs_upload_template_checkpointed(ctx._h, C.byref(cs), C.byref(cp), hp, C.byref(ck), C.byref(h))
    else:
        st = lib.bpg_r1cs_upload_template_hinted(ctx._h, C.byref(cs), C.byref(cp), hp, C.byref(h))
    assert st == 0, lib.bpg_last_error()
    return bpg.ResidentCircuit(ctx, h, inst.n, inst.m, n_params=len(prog.param_rows), q=inst.q, n_ck=len(ck_vars), n_inputs=len(it.inputs) if public else 0), it, levels


WITNESS_KERNELS = ("k_witness_eval_batch", "k_witness_eval", "k_witness_ck_verify_batch", "k_witness_ck_verify", "k_input_slots", "k_bt_commit_v")


def launches(ctx, fn):
    """fn() under the all-kernels profile -> (its result, launches of the witness kernels)"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: rep.get(k, {"count": 0})["count"] for k in WITNESS_KERNELS}


def bumped(x):
    return RT.sc(int.from_bytes(x, "little") + 1)


def refused(call, word=None):
    with pytest.raises(bpg.BpgError) as e:
        call()
    assert e.value.status == INVALID and (word is None or word in str(e.value)), str(e.value)


# ------------------------------------------------------------------------------------------------ the scenarios (shared with the child process)
def scenario_assign(ctx, hosts, seed, value_seeds=(1, 2, 3)):
    tmpl, it0, _ = upload(ctx, seed)
    try:
        with pytest.raises(bpg.BpgError) as e:                                   # uploaded without a witness: nothing to prove yet
            tmpl.prove(hosts.pre, bytes(32 * tmpl.m), rng("none"))
        assert e.value.status == MISSING
        for vs in value_seeds:
            h = hosts(seed, vs)
            tmpl.assign(h.inst.v, h.params)
            got = h.prove_on(tmpl)
            assert got == h.proof(), "shape %d, witness %d: the assigned template and the host assembly give different proofs" % (seed, vs)
            assert tmpl.verify(h.state, h.coms, got[0]) == 0 and tmpl.check().ok, "shape %d, witness %d" % (seed, vs)
            if h.N <= ORACLE_N:
                assert h.oracle_accepts(got[0]), "shape %d, witness %d: the oracle rejects the proof" % (seed, vs)
            for j in {0, len(h.params) - 1} if h.params else ():                  # one parameter bumped: exactly its row, and a statement the proof does not prove
                bad = list(h.params); bad[j] = bumped(bad[j])
                tmpl.assign(h.inst.v, bad)
                rep = tmpl.check()
                assert (rep.bad_rows, rep.rows, rep.bad_multipliers) == (1, [it0.rows[j]], 0), "shape %d, witness %d, parameter %d: %r" % (seed, vs, j, rep)
                assert h.prove_on(tmpl) == got and tmpl.verify(h.state, h.coms, got[0]) == 3
                tmpl.assign(h.inst.v, h.params)                                  # ... and a correct assign heals it
                assert tmpl.check().ok and tmpl.verify(h.state, h.coms, got[0]) == 0
    finally:
        tmpl.free()


def scenario_lockstep(ctx, hosts, seed, Ks=(1, 5, 65), waves_per_item=False):
    tmpl, _, levels = upload(ctx, seed)
    try:
        for K in Ks:
            hs = [hosts(seed, 1 + k) for k in range(K)]
            flags = [k % 4 if K == 5 else 0 for k in range(K)]                   # the batch of five mixes the dialects
            waves = K if waves_per_item else 1
            res, n = launches(ctx, lambda: tmpl.prove_batch([h.batch_item(flags=f) for h, f in zip(hs, flags)]))
            assert n["k_witness_eval_batch"] == levels * waves and n["k_witness_eval"] == 0, "shape %d, K = %d: %r" % (seed, K, n)
            assert res == [h.result(False, f) for h, f in zip(hs, flags)], "shape %d, K = %d: prove_batch differs from the host assemblies' proofs" % (seed, K)
            res, n = launches(ctx, lambda: tmpl.prove_batch_commit([h.batch_item(True, f, hosts.pre) for h, f in zip(hs, flags)]))
            assert n["k_witness_eval_batch"] == levels * waves and n["k_witness_eval"] == 0 and n["k_bt_commit_v"] == (waves if tmpl.m else n["k_bt_commit_v"]), \
                "shape %d, K = %d: %r" % (seed, K, n)
            assert res == [h.result(True, f) for h, f in zip(hs, flags)], "shape %d, K = %d: prove_batch_commit differs from the host assemblies' proofs" % (seed, K)
            for h in hs[:3]:
                v, vb = h.inst.v, h.inst.v_blinding
                want = ctx.pedersen_commit([v[32 * i:32 * i + 32] for i in range(tmpl.m)], [vb[32 * i:32 * i + 32] for i in range(tmpl.m)]) if tmpl.m else []
                assert h.coms == b"".join(want)
        with pytest.raises(bpg.BpgError) as e:                                   # no witness left behind
            tmpl.prove(hosts.pre, bytes(32 * tmpl.m), rng("none"))
        assert e.value.status == MISSING
    finally:
        tmpl.free()


def nothing_is_written_for(ctx, tmpl, items, bad_at, commit):
    """the C call itself on buffers filled with 0xa5: the failed item's transcript, proof buffer, proof length and commitments are left exactly as given"""
    K, nb = len(items), max(32 * tmpl.m, 1)
    arr, keep = tmpl._template_items([it[:6] for it in items], bpg._TemplateCkItem)
    coms = [C.create_string_buffer(b"\xa5" * nb, nb) for _ in range(K)]
    firsts = [C.c_uint64(7) for _ in range(K)]
    cks = [b"".join(it[6]) for it in items]
    for k in range(K):
        C.memset(keep[k][1], 0xa5, len(keep[k][1]))
        arr[k].ck_values = cks[k]; arr[k].first_mismatch = C.pointer(firsts[k])
        if commit:
            arr[k].commitments_out = C.cast(coms[k], C.c_void_p)
    status = (C.c_int32 * K)(*[77] * K)
    rc = bpg.lib().bpg_r1cs_prove_template_batch_checkpointed(ctx._h, tmpl._h, C.c_uint64(K), arr, C.c_int32(1 if commit else 0), status)
    assert rc == MISMATCH and [s for s in status] == [MISMATCH if k == bad_at else 0 for k in range(K)], (rc, list(status))
    ts, out, ln = keep[bad_at][:3]
    assert ts.raw[:203] == items[bad_at][2] and out.raw == b"\xa5" * len(out) and ln.value == len(out) and coms[bad_at].raw == b"\xa5" * nb
    assert all(keep[k][1].raw != b"\xa5" * len(keep[k][1]) for k in range(K) if k != bad_at)


def scenario_checkpoints(ctx, hosts, seed, density, K=5):
    refs, R = RT.checkpoint_set(seed, density, RT.mul_refs(RT.shape(seed).n))
    tmpl, it0, levels = upload(ctx, seed, checkpoints=refs)
    try:
        assert tmpl.n_ck == len(refs) > 0
        hs = [hosts(seed, 1 + k) for k in range(K)]
        cks = [h.items[0].checkpoints(refs)[1] for h in hs]
        h = hs[0]
        tmpl.assign(h.inst.v, h.params, checkpoints=cks[0])
        assert h.prove_on(tmpl) == h.proof(), "shape %d, density %s: the checkpointed assign and the host assembly give different proofs" % (seed, density)
        assert tmpl.verify(h.state, h.coms, h.proof()[0]) == 0 and tmpl.check().ok
        bad_at, k = K - 2, R.randrange(len(refs))                                # one item carries one bumped value
        wrong = list(cks[bad_at]); wrong[k] = bumped(wrong[k])
        first_bad = RT.first_mismatch(it0.shape, hs[bad_at].items[0].v, (), refs, [int.from_bytes(x, "little") for x in wrong])
        assert first_bad is not None and first_bad <= k
        for commit in (False, True):
            items = [x.batch_item(commit, 0, hosts.pre) + (ck,) for x, ck in zip(hs, cks)]
            res, n = launches(ctx, lambda: tmpl.prove_batch_checkpointed(items, commit=commit))
            assert n["k_witness_eval_batch"] == levels and n["k_witness_ck_verify_batch"] == 1 and n["k_witness_eval"] == 0, "shape %d: %r" % (seed, n)
            assert res == [x.result(commit) for x in hs], "shape %d, density %s: the checkpointed batch differs from the host assemblies' proofs" % (seed, density)
            items[bad_at] = items[bad_at][:6] + (wrong,)
            res, st, first = tmpl.prove_batch_checkpointed(items, commit=commit, return_status=True)
            assert st == [MISMATCH if i == bad_at else 0 for i in range(K)], "shape %d, density %s: %r" % (seed, density, st)
            assert first == [first_bad if i == bad_at else None for i in range(K)], "shape %d, density %s, checkpoint %d bumped: %r" % (seed, density, k, first)
            for i, x in enumerate(hs):                                           # the item alone fails, nothing of it is returned, the others are proved
                assert res[i] == (((None, hosts.pre, None) if commit else (None, x.state)) if i == bad_at else x.result(commit)), "shape %d, item %d" % (seed, i)
            nothing_is_written_for(ctx, tmpl, items, bad_at, commit)
        with pytest.raises(bpg.BpgError) as e:
            tmpl.assign(hs[bad_at].inst.v, hs[bad_at].params, checkpoints=wrong)
        assert e.value.status == MISMATCH and e.value.first_mismatch == first_bad
        with pytest.raises(bpg.BpgError) as e:
            hs[bad_at].prove_on(tmpl)
        assert e.value.status == MISSING
        refused(lambda: tmpl.prove_batch([h.batch_item()]))                       # the older batch call refuses a checkpointed template
    finally:
        tmpl.free()


def scenario_inputs(ctx, hosts, seed, checkpoints=(), Ks=(1, 5)):
    tmpl, it0, levels = upload(ctx, seed, checkpoints=checkpoints, public=True)
    try:
        assert tmpl.n_inputs == len(it0.inputs) > 0
        hs = [hosts(seed, 1 + k, public=True) for k in range(max(Ks))]
        cks = [h.items[0].checkpoints(checkpoints)[1] if checkpoints else None for h in hs]
        for h, ck in zip(hs[:3], cks):
            tmpl.assign(h.inst.v, h.params, checkpoints=ck, inputs=h.items[0].inputs)
            got = h.prove_on(tmpl)
            assert got == h.proof(), "shape %d: the template under public inputs and the assembly with the constants baked in give different proofs" % seed
            assert tmpl.verify(h.state, h.coms, got[0]) == 0 and tmpl.check().ok, "shape %d" % seed
            if h.N <= ORACLE_N:
                assert h.oracle_accepts(got[0]), "shape %d: the oracle rejects the proof" % seed
        for K in Ks:
            for commit in (False, True):
                items = [h.batch_item(commit, 0, hosts.pre) + (ck, h.items[0].inputs) for h, ck in zip(hs[:K], cks)]
                res, n = launches(ctx, lambda: tmpl.prove_batch_inputs(items, commit=commit))
                assert n["k_witness_eval_batch"] == levels and n["k_witness_eval"] == 0, "shape %d, K = %d: %r" % (seed, K, n)
                assert res == [h.result(commit) for h in hs[:K]], "shape %d, K = %d: the batch with inputs differs from the baked assemblies' proofs" % (seed, K)
        h = hs[0]                                                                # the calls that refuse a template with inputs, by contract
        refused(lambda: tmpl.assign(h.inst.v, h.params), "public inputs")
        refused(lambda: tmpl.prove_batch([h.batch_item()]), "public inputs")
        refused(lambda: tmpl.prove_batch_commit([h.batch_item(True, 0, hosts.pre)]))
        refused(lambda: tmpl.repeat(2), "public inputs")
        refused(lambda: tmpl.check_batch([(h.inst.v, h.params)]))
        refused(lambda: ctx.join([(tmpl, 1)]))
    finally:
        tmpl.free()


def scenario_repeat(ctx, seed, K):
    tmpl, it0, levels = upload(ctx, seed, witness=True)
    sh = it0.shape
    host = Host(ctx, lambda p: [RT.item(p, seed, 10 + k) for k in range(K)], ("repeat", seed, K))
    per_item = [(it.values, it.params) for it in host.items]
    try:
        if sh.rows:                                                              # check_batch: item K - 1 alone is bad, at the row of its bumped parameter
            bad = list(per_item); bad[-1] = (bad[-1][0], bad[-1][1][:-1] + [bumped(bad[-1][1][-1])])
            assert tmpl.check_batch(bad) == [[] for _ in range(K - 1)] + [[it0.rows[-1]]], "shape %d, K = %d" % (seed, K)
        assert tmpl.check_batch(per_item) == [[] for _ in range(K)]
        rep = tmpl.repeat(K)
    finally:
        tmpl.free()                                                              # the source is gone before the repeat is used
    try:
        assert (rep.n, rep.m, rep.n_params, rep.q) == (host.inst.n, host.inst.m, K * sh.rows, host.inst.q) == (K * sh.n, K * sh.m, K * sh.rows, K * sh.q)
        ctx.profile_set(2)
        rep.assign(host.inst.v, host.params)
        counts = ctx.profile_report(); ctx.profile_set(0)
        assert counts.get("k_witness_eval_repeat", {"count": 0})["count"] == levels and "k_witness_eval" not in counts, counts
        got = host.prove_on(rep)
        assert got == host.proof(), "shape %d, K = %d: the repeat and the K-fold one-prover assembly give different proofs" % (seed, K)
        assert rep.verify(host.state, host.coms, got[0]) == 0 and rep.check().ok
        if host.N <= ORACLE_N:
            assert host.oracle_accepts(got[0])
        if sh.rows:
            bad = list(host.params); bad[-1] = bumped(bad[-1])
            rep.assign(host.inst.v, bad)
            report = rep.check()
            assert report.items(sh.q) == [(K - 1, it0.rows[-1])] and report.bad_rows == 1 and report.bad_multipliers == 0, "shape %d, K = %d: %r" % (seed, K, report)
            assert rep.verify(host.state, host.coms, got[0]) == 3
    finally:
        rep.free()


# (shape seed, count, checkpointed): a part with m = 0 and no rows at all (45) in the middle, without checkpoints between two parts with; counts {1, 3, 2}
JOINS = {
    "plain between checkpointed": [(35, 1, True), (45, 3, False), (13, 2, True)],
    "two parts": [(112, 2, False), (9, 1, False)],
    "sixty-five and a hinted single": [(31, 3, False), (118, 1, False), (22, 2, True)],
}


def scenario_join(ctx, parts, tag):
    sources, cks_of = [], []
    try:
        for seed, count, ck in parts:
            refs = RT.checkpoint_set(seed, 0.5, RT.mul_refs(RT.shape(seed).n))[0] if ck else []
            sources.append(upload(ctx, seed, checkpoints=refs, witness=True))
            cks_of.append(refs)
        j = ctx.join([(t, count) for (t, _, _), (_, count, _) in zip(sources, parts)])
    finally:
        for t, _, _ in sources:
            t.free()                                                             # every source is gone before the first assign
    try:
        host = Host(ctx, lambda p: [RT.item(p, seed, 100 + 10 * k + i) for k, (seed, count, _) in enumerate(parts) for i in range(count)], ("join", tag))
        ck_values, at = [], 0
        for (seed, count, _), refs in zip(parts, cks_of):
            for it in host.items[at:at + count]:
                ck_values += it.checkpoints(refs)[1]
            at += count
        assert (j.n, j.m, j.q, j.n_params, j.n_ck) == (host.inst.n, host.inst.m, host.inst.q, len(host.params), len(ck_values))
        ctx.profile_set(2)
        j.assign(host.inst.v, host.params, checkpoints=ck_values if ck_values else None)
        counts = ctx.profile_report(); ctx.profile_set(0)
        assert counts.get("k_witness_eval_join", {"count": 0})["count"] == max(levels for _, _, levels in sources), counts    # the MOST levels any part has
        assert "k_witness_eval" not in counts and "k_witness_eval_repeat" not in counts, counts
        got = host.prove_on(j)
        assert got == host.proof(), "join %r: the join and the one-prover assembly give different proofs" % (parts,)
        assert j.verify(host.state, host.coms, got[0]) == 0 and j.check().ok
        if host.N <= ORACLE_N:
            assert host.oracle_accepts(got[0])
        bad = list(host.params); bad[-1] = bumped(bad[-1])                        # one parameter of the last part's last item
        j.assign(host.inst.v, bad, checkpoints=ck_values if ck_values else None)
        report = j.check()
        last = sources[-1][1]
        assert report.parts(j.layout) == [(len(parts) - 1, parts[-1][1] - 1, last.rows[-1])] and report.bad_rows == 1 and report.bad_multipliers == 0, report
        assert j.verify(host.state, host.coms, got[0]) == 3
        if ck_values:                                                            # a wrong checkpoint value: the place in the joined list, and no witness afterwards
            wrong = list(ck_values); wrong[-1] = bumped(wrong[-1])
            with pytest.raises(bpg.BpgError) as e:
                j.assign(host.inst.v, host.params, checkpoints=wrong)
            part = max(k for k, refs in enumerate(cks_of) if refs)               # the last value of the joined list: the last item of the last checkpointed part
            assert e.value.status == MISMATCH and e.value.first_mismatch <= len(wrong) - 1 and e.value.place[:2] == (part, parts[part][1] - 1), str(e.value)
    finally:
        j.free()


# ------------------------------------------------------------------------------------------------ the child process of test_nothing_is_left_behind
def _child():
    ctx = bpg.Context(0)
    ctx.gens_ensure(CAPACITY)
    hosts = Hosts(ctx)
    scenario_assign(ctx, hosts, 18, value_seeds=(1,))
    scenario_lockstep(ctx, hosts, 18, Ks=(5,))
    scenario_checkpoints(ctx, hosts, 18, 0.5, K=3)
    scenario_inputs(ctx, hosts, 10, Ks=(1,))
    scenario_repeat(ctx, 73, 2)
    scenario_join(ctx, JOINS["plain between checkpointed"], "child")
    with_open = bpg.live_resources()
    hosts.have.clear()
    ctx.close()
    print(json.dumps({"open": [with_open[k] for k in bpg.LIVE_RESOURCE_KEYS], "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}))


if __name__ == "__main__":
    _child()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(CAPACITY)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hosts(ctx):
    return Hosts(ctx)


def shown(seed, fn, public=False):
    """fn(); a failure prints the shape and its schedule first (the CPU hooks evaluate the same shape: host against device localises it)"""
    try:
        fn()
    except BaseException:
        inst, prog, hints, it = stub(seed, public)
        print(RT.describe(it.shape))
        print(json.dumps(schedule_inputs((inst, prog, hints, it.inputs), len(it.inputs)) if public else schedule_hinted(inst, prog, hints)))
        raise


def test_the_pinned_shapes_cover_the_edges():
    shapes = [RT.shape(s) for s in PINNED]
    levels = {s: schedule_hinted(*stub(s)[:3])["levels"] for s in PINNED}
    assert {1, 2, 3} <= {sh.n for sh in shapes} and {17, 33, 65} & {sh.n for sh in shapes} and all(sh.n <= 256 for sh in shapes)
    assert any(sh.m == 0 for sh in shapes) and any(sh.q == 0 for sh in shapes) and max(levels.values()) >= 10
    assert any(sh.hints and max(sh.hint_bits) >= 200 for sh in shapes) and any(sh.rows >= 4 for sh in shapes)
    assert all(RT.shape(s, True).n_inputs for s in PINNED_PUBLIC) and {1, 2, 3, 17, 33, 65, 200} <= {RT.shape(s, True).n for s in PINNED_PUBLIC}


@pytest.mark.parametrize("seed", PINNED)
def test_assign(ctx, hosts, seed):
    shown(seed, lambda: scenario_assign(ctx, hosts, seed))


def test_assign_rebuilds_the_merge_sets(monkeypatch):
    """BPG_MERGE=1 and BPG_TT_ORIG_LG=0 put the proof on the path that groups equal scalars once per resident witness (bit vectors: large groups); a set that
    survived the assign would give a wrong A_I without any error.  Shape 22: 32 of its 65 multipliers are bit hints."""
    monkeypatch.setenv("BPG_MERGE", "1"); monkeypatch.setenv("BPG_TT_ORIG_LG", "0")
    own = bpg.Context(0)
    tmpl = None
    try:
        own.gens_ensure(128)
        hs = Hosts(own)
        tmpl, _, _ = upload(own, 22)
        first, second = hs(22, 1), hs(22, 2)
        tmpl.assign(first.inst.v, first.params)
        assert first.prove_on(tmpl) == first.proof()
        assert own.schedule()["merge_equal"] == 1 and own.schedule()["merged_skipped_last"] > 0, "this path must really build merge sets"
        assert first.prove_on(tmpl) == first.proof()                             # ... again, with this witness's sets in place
        rc, proof, state = O.prove(O.Gens(128), first.state, to_oracle(first.inst), first.inst.v_blinding, rng(first.tag), O.FLAG_FAST_MSM)
        assert rc == 0 and (proof, state) == first.proof()                       # the yardstick itself ran under the merge: the oracle pins it
        tmpl.assign(second.inst.v, second.params)
        assert second.prove_on(tmpl) == second.proof()
        tmpl.assign(first.inst.v, first.params)
        assert first.prove_on(tmpl) == first.proof()
    finally:
        if tmpl is not None:
            tmpl.free()
        own.close()


@pytest.mark.parametrize("seed", PINNED)
def test_lockstep(ctx, hosts, seed):
    shown(seed, lambda: scenario_lockstep(ctx, hosts, seed))


def test_lockstep_one_item_per_wave(monkeypatch):
    """BPG_BATCH_WAVE_MB=0: one proof per wave - levels x K launches"""
    monkeypatch.setenv("BPG_BATCH_WAVE_MB", "0")
    own = bpg.Context(0)
    try:
        own.gens_ensure(64)
        scenario_lockstep(own, Hosts(own), 9, Ks=(5,), waves_per_item=True)
    finally:
        own.close()


@pytest.mark.parametrize("density", [0.5, 1.0])
@pytest.mark.parametrize("seed", PINNED)
def test_checkpoints(ctx, hosts, seed, density):
    shown(seed, lambda: scenario_checkpoints(ctx, hosts, seed, density))


@pytest.mark.parametrize("seed", PINNED_PUBLIC)
def test_public_inputs(ctx, hosts, seed):
    shown(seed, lambda: scenario_inputs(ctx, hosts, seed), public=True)


def test_public_inputs_and_checkpoints_together(ctx, hosts):
    seed = 10
    scenario_inputs(ctx, hosts, seed, checkpoints=RT.checkpoint_set(seed, 0.5, RT.mul_refs(RT.shape(seed, True).n))[0])


# 65 copies (one more than a block of the lane map holds) of the shapes of n <= 3: 195 multipliers at most
@pytest.mark.parametrize("seed,K", [(s, K) for s in PINNED for K in (1, 2, 3)] + [(s, 65) for s in SMALL])
def test_repeat(ctx, seed, K):
    shown(seed, lambda: scenario_repeat(ctx, seed, K))


@pytest.mark.parametrize("name", list(JOINS))
def test_join(ctx, name):
    scenario_join(ctx, JOINS[name], name)


def test_nothing_is_left_behind():
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "leak"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["open"][0] > 0 and out["end"] == [0] * 6, out
