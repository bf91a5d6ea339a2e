"""Lockstep verification on the GPU (bpg_r1cs_verify_resident_batch, csrc/hip/k_vwave.cuh): K proofs of ONE resident circuit with a constant number of launches
per wave.  Proofs come from the CPU oracle (tests/verify_cases.py) or, for the templates with public inputs, from prove_batch_inputs; every status is held against
bpg_r1cs_verify_resident on the item alone, every accepted call against the profile (ONE bucket sweep: no item-by-item pass behind which a wrong accumulator
could hide), and the wave kernels against the integer model of tests/verify_wave_cases.py byte for byte.

Run as a script (`python tests/test_verify_wave_gpu.py leak`) the file runs an accepted call, a rejected call with per-item constants and the hook in a process
of its own, frees everything and prints the census of what the process still holds (bpg_test_live_resources)."""
import json
import pathlib
import subprocess
import sys

if __name__ == "__main__":
    _root = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "tests"), str(_root / "tests" / "golden")]

import collections
import ctypes as C
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
import template_inputs_cases as TC
import verify_cases as VC
import verify_wave_cases as W
from template_inputs_cases import sc, rng

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
BATCH_SEED = hashlib.sha256(b"verify wave batch").digest()
VW = ("k_vw_exp", "k_vw_tails", "k_vw_flatten", "k_vw_small", "k_vw_scalars", "k_vw_reduce")
PER_ITEM = ("k_exp_table", "k_flatten", "k_flatten_const", "k_ipa_s", "k_verify_scalars", "k_verify_scalars_acc", "k_reduce_partials")
MSM_PREFIXES = ("k_msm_", "k_scan_", "k_bucket_", "k_window_")


def vseed(k):
    return hashlib.sha256(b"verify wave seed %d" % k).digest()


def alone(ctx, res, state, V, proof, seed, flags):
    """bpg_r1cs_verify_resident -> (status, transcript state after)"""
    ts = C.create_string_buffer(bytes(state), 203)
    s = bpg.lib().bpg_r1cs_verify_resident(ctx._h, res._h, ts, C.c_uint64(res.m), V, proof, C.c_uint64(len(proof)), seed, C.c_uint32(flags))
    return s, ts.raw[:203]


def launches(ctx, fn):
    """fn() under the all-kernels profile -> (its result, {kernel: launches})"""
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: v["count"] for k, v in rep.items()}


def hook(res, records, **kw):
    return res.test_verify_wave_scalars([W.record_bytes(r) for r in records], **kw)


def against_model(res, circs, records, **kw):
    """the hook's accumulators and slots against the integer model, byte for byte -> the evidence"""
    g, h, slots, ev = hook(res, records, **kw)
    wg, wh, wslots = W.wave_bytes(circs, records)
    assert g == wg and h == wh, "accumulators"
    assert slots == wslots, "slots [w_V | w_c | delta]"
    return ev


# ------------------------------------------------------------------------------------------------ the leak scenario (child process)
class Inputs:
    """K statements of one gadget with a public side: ONE template, the host assemblies with the values baked in, the proofs of prove_batch_inputs"""
    def __init__(self, ctx, name, args):
        fn = TC.GADGETS[name][0]
        self.name, self.args = name, args
        self.tmpl = fn(ctx, *args[0], True, tag="vw-%s-t" % name).prover.template(ctx)
        self.cases = [fn(ctx, *a, False, tag="vw-%s-%d" % (name, k)) for k, a in enumerate(args)]
        self.inst = [c.prover.instance() for c in self.cases]
        self.state = [c.transcript.state for c in self.cases]
        self.coms = [b"".join(c.commitments) for c in self.cases]
        self.inputs = [b"".join(fn(None, *a, True, tag="vw-%s-%d" % (name, k), prover_cls=TC.StubProver).inputs) for k, a in enumerate(args)]
        items = [(i.v, [], s, i.v_blinding, rng("vw %s %d" % (name, k)), 0, None, [inp[32 * j:32 * j + 32] for j in range(len(inp) // 32)])
                 for k, (i, s, inp) in enumerate(zip(self.inst, self.state, self.inputs))]
        self.proofs = [r[0] for r in self.tmpl.prove_batch_inputs(items, commit=False)]
        self.rows = [W.Rows(i) for i in self.inst]

    def items(self, order=None, inputs=None):
        """the call's items; inputs[k]: the input bytes item k brings (default: its own; None: the standing slots)"""
        order = range(len(self.args)) if order is None else order
        inputs = {} if inputs is None else inputs
        return [(self.state[k], self.coms[k], self.proofs[k], vseed(k), 0, None, inputs.get(k, self.inputs[k])) for k in order]

    def free(self):
        self.tmpl.free()


LT_ARGS = [(5 + 3 * k, b) for k, b in enumerate([1000, 9, 2**64 + 1, 2**126 - 1, 77, 2**100, 12345, 2**32])]
NE_ARGS = [(10 + k, r) for k, r in enumerate([3, 2**130 + 6, 7, 0, 2**200, 5, 99, 2**64])]


def _child():
    ctx = bpg.Context(0)
    ctx.gens_ensure(512)
    lt = Inputs(ctx, "less_than", LT_ARGS[:3])
    ok = lt.tmpl.verify_batch(lt.items(), batch_seed=BATCH_SEED)[0] == [0, 0, 0]
    ok = ok and lt.tmpl.verify_batch(lt.items(inputs={1: lt.inputs[0]}), batch_seed=BATCH_SEED)[0] == [0, 3, 0]
    recs = W.challenge_set("hashed", 9, 3)
    ok = ok and hook(lt.tmpl, recs, inputs=lt.inputs)[2] == W.wave_bytes(lt.rows, recs)[2]
    with_open = bpg.live_resources()
    lt.free(); ctx.close()
    print(json.dumps({"ok": ok, "open": [with_open[k] for k in bpg.LIVE_RESOURCE_KEYS], "end": [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]}))


if __name__ == "__main__":
    _child()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus(ctx):
    """the six circuits of verify_cases, each resident; their base proofs and mutants; what bpg_r1cs_verify_resident leaves of an accepted base proof"""
    circs, bases, mutants = VC.corpus()
    assert list(circs) == ["range8", "range56", "small5", "one", "none", "big"]
    res = {name: ctx.upload(c.instance(witness=False)) for name, c in circs.items()}
    by_circuit = collections.OrderedDict((name, [r for r in bases if r.base.split("/")[0] == name]) for name in circs)
    assert all(len(v) == 4 and [r.flags for r in v] == [0, 1, 2, 3] for v in by_circuit.values())
    yield circs, by_circuit, mutants, res
    for r in res.values():
        r.free()


@pytest.fixture
def make_ctx(monkeypatch):
    """A fresh context with the given environment knobs (they are read once, at context creation)."""
    made = []

    def make(cap=1024, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        c = bpg.Context(0)
        made.append(c)
        for k in env:
            monkeypatch.delenv(k)
        c.gens_ensure(cap)
        return c
    yield make
    for c in made:
        c.close()


# ------------------------------------------------------------------------------------------------ 1. good items: the one MSM accepts them
def test_good_items_are_accepted_by_the_one_msm(ctx, corpus):
    """per circuit the four dialect base proofs twice, under eight verifier seeds, in one call: N = 1 (no L, R), 5 -> 8, 56 -> 64, 700 -> 1024 (four blocks of
    lanes on both sides of `real`); the n = 0 circuit is served item by item and left out of the launch counts"""
    circs, by_circuit, _, res = corpus
    assert len(circs) == 6
    waved = 0
    for name, bases in by_circuit.items():
        r = res[name]
        recs = bases + bases
        items = [(b.state, b.V, b.proof, vseed(k), b.flags) for k, b in enumerate(recs)]
        want = [alone(ctx, r, *it) for it in items]
        assert [w[0] for w in want] == [0] * 8
        (rc, st, states), counts = launches(ctx, lambda: r.verify_batch(items, batch_seed=BATCH_SEED, return_status=True))
        assert rc == 0 and st == [0] * 8, (name, st)
        assert states == [w[1] for w in want], name
        if circs[name].n == 0:                                                    # the existing path, item by item: eight sums of their own
            assert not any(k in counts for k in VW) and counts["k_bucket_chunks"] == counts["k_verify_scalars"] == 8, (name, counts)
            continue
        assert "k_verify_scalars" not in counts and "k_verify_scalars_acc" not in counts, (name, counts)
        assert counts["k_bucket_chunks"] == 1, (name, counts)                     # ONE sweep: the weighted sum itself was the identity
        assert counts["k_decompress"] == 1 and not any(k in counts for k in PER_ITEM), (name, counts)
        ev = hook(r, W.challenge_set("hashed", circs[name].lgN, 8))[3]
        assert ev["count"] == 8 and ev["launches"]["k_vw_tails"] == 0 and all(ev["launches"][k] == ev["waves"] for k in VW if k != "k_vw_tails"), ev
        assert {k: counts.get(k, 0) for k in VW} == ev["launches"], (name, counts, ev)
        waved += 1
    assert waved == 5
    assert res["range8"].verify_batch([]) == ([], [])                             # count = 0: BPG_OK, nothing launched


# ------------------------------------------------------------------------------------------------ 2. launches do not grow with K
def test_launches_do_not_grow_with_the_batch(ctx, corpus):
    """8 and 256 copies of the range56 proof: the same launches, kernel by kernel - the wave's, the decoder's and those of the one MSM"""
    _, by_circuit, _, res = corpus
    b = by_circuit["range56"][0]
    r = res["range56"]
    r.verify_batch([(b.state, b.V, b.proof, vseed(0), b.flags)] * 8, batch_seed=BATCH_SEED)          # warm: buffers grown
    out = {}
    for K in (8, 256):
        items = [(b.state, b.V, b.proof, vseed(k), b.flags) for k in range(K)]
        (st, _), counts = launches(ctx, lambda: r.verify_batch(items, batch_seed=BATCH_SEED))
        assert st == [0] * K
        print("K = %d: %s" % (K, counts))
        assert counts["k_bucket_chunks"] == 1
        out[K] = counts
    assert out[8] == out[256] and all(out[8][k] == 1 for k in VW if k != "k_vw_tails"), out
    assert {k for k in out[8] if not k.startswith(MSM_PREFIXES)} == {"k_decompress"} | (set(VW) - {"k_vw_tails"}), out


# ------------------------------------------------------------------------------------------------ 3. mutants among good proofs, one call per circuit
def pick_mutants(mutants):
    """one mutant per (field kind x class), walking through the bases so that dialects vary (the rule of test_verify_malformed_gpu.pick_mutants)"""
    cells = collections.OrderedDict()
    for r in mutants:
        if r.cls != "capacity":
            cells.setdefault((r.kind, r.cls), []).append(r)
    return [c[(7 * k) % len(c)] for k, c in enumerate(cells.values())]


def test_mutants_among_good_proofs_in_one_call(ctx, corpus):
    circs, by_circuit, mutants, res = corpus
    total, other_statements = 0, 0
    for name, bases in by_circuit.items():
        mine = [r for r in mutants if r.base.split("/")[0] == name]
        picked = pick_mutants(mine)
        want_cells = {(r.kind, r.cls) for r in mine if r.cls != "capacity"}
        assert {(r.kind, r.cls) for r in picked} == want_cells and len(picked) == len(want_cells) >= 40, (name, len(picked))
        vinst = bases[0].circuit
        assert all(b.circuit is vinst for b in bases)
        here = [r for r in picked if r.circuit is vinst]
        recs = bases[:2] + here + bases[2:]                                      # good proofs in front, behind, and none between: ONE call
        items = [(r.state, r.V, r.proof, r.seed, r.flags) for r in recs]
        want = [alone(ctx, res[name], *it) for it in items]
        rc, st, states = res[name].verify_batch(items, batch_seed=BATCH_SEED, return_status=True)
        assert st == [VC.expected_status(r) for r in recs] == [w[0] for w in want] == [r.status for r in recs], name
        assert states == [w[1] for w in want], name
        assert rc == next(s for s in st if s), name                              # the status of the first failing item
        total += len(here)
        # a mutant whose STATEMENT has other rows is a good proof against another circuit: that circuit resident, the mutant among copies of itself
        for r in picked:
            if r.circuit is vinst:
                continue
            other = ctx.upload(r.circuit)
            try:
                items = [(r.state, r.V, r.proof, vseed(k), r.flags) for k in range(3)]
                want = [alone(ctx, other, *it) for it in items]
                st, states = other.verify_batch(items, batch_seed=BATCH_SEED)
                assert st == [VC.expected_status(r)] * 3 == [w[0] for w in want] and states == [w[1] for w in want], r.name
            finally:
                other.free()
            other_statements += 1
    assert total >= 6 * 40 and other_statements >= 6, (total, other_statements)


def test_capacity_mutants_on_a_context_of_too_few_generators(corpus):
    circs, by_circuit, mutants, _ = corpus
    caps = sorted({r.capacity for r in mutants if r.cls == "capacity"})
    assert caps == [4, 512]
    seen = 0
    for cap in caps:
        c2 = bpg.Context(0)
        try:
            c2.gens_ensure(cap)
            for name in circs:
                recs = [r for r in mutants if r.cls == "capacity" and r.capacity == cap and r.base.split("/")[0] == name]
                if not recs:
                    continue
                r2 = c2.upload(recs[0].circuit)
                try:
                    items = [(r.state, r.V, r.proof, r.seed, r.flags) for r in recs]
                    st, states = r2.verify_batch(items, batch_seed=BATCH_SEED)
                    assert st == [1] * len(recs) == [VC.expected_status(r) for r in recs] == [alone(c2, r2, *it)[0] for it in items], (cap, name)
                    assert states == [r.state for r in recs]                     # refused before the transcript is touched
                finally:
                    r2.free()
                seen += len(recs)
        finally:
            c2.close()
    assert seen == sum(r.cls == "capacity" for r in mutants) == 4 * 4 + 4


# ------------------------------------------------------------------------------------------------ 4. the cancelling pair
def test_weights_defeat_a_cancelling_pair(ctx, corpus):
    """a is never absorbed into the transcript: copies with a + 1 and a - 1 see the same challenges and their residuals are +Q and -Q"""
    _, by_circuit, mutants, res = corpus
    by_name = {r.name: r for r in mutants}
    by_name.update({r.name: r for v in by_circuit.values() for r in v})
    for base in ("small5/f0", "small5/f3", "big/f1", "one/f0", "range56/f2"):
        recs = [by_name[base + "/a=plus_1"], by_name[base + "/a=minus_1"], by_name[base]]
        for seed in (bytes(32), BATCH_SEED):
            st, _ = res[base.split("/")[0]].verify_batch([(r.state, r.V, r.proof, r.seed, r.flags) for r in recs], batch_seed=seed)
            assert st == [3, 3, 0], base


# ------------------------------------------------------------------------------------------------ 5. the kernels against the integer model
@pytest.fixture(scope="module")
def model_circuits():
    out = W.model_circuits()
    assert len(out) == 25 + 5
    return out


def _model_pass(c, model_circuits, waves):
    done = 0
    for name, circ in model_circuits:
        r = c.upload(circ.instance(witness=False))
        try:
            for set_name in W.SET_NAMES:
                recs = W.challenge_set(set_name, circ.lgN, W.K_MODEL, name.encode())
                ev = against_model(r, [circ] * W.K_MODEL, recs)
                assert ev["waves"] == waves and ev["count"] == 3 and ev["N"] == circ.N, (name, ev)
                done += 1
        finally:
            r.free()
    return done


def test_wave_kernels_equal_the_integer_model(ctx, model_circuits):
    assert _model_pass(ctx, model_circuits, 1) == 30 * 3


def test_wave_kernels_equal_the_integer_model_in_three_waves(make_ctx, model_circuits):
    """BPG_BATCH_WAVE_MB=0: one item per wave, the accumulators carried from wave to wave"""
    assert _model_pass(make_ctx(BPG_BATCH_WAVE_MB=0), model_circuits, 3) == 30 * 3


def test_wave_kernels_at_the_chunk_edges(ctx, corpus):
    """more items than the block target wants chunks: a chunk holds two items and the last one is ragged (K = target + 1) or full (K = 2 x target); and, from that
    evidence, K = items-per-chunk and items-per-chunk + 1"""
    circs, _, _, res = corpus
    for name in ("small5", "range56"):
        circ, r = circs[name], res[name]
        target = hook(r, W.challenge_set("hashed", circ.lgN, 1))[3]["target_blocks"]
        assert target >= 4
        seen = []
        for K in (target + 1, 2 * target) if name == "small5" else (target + 1,):
            recs = W.challenge_set("edges" if K % 2 else "hashed", circ.lgN, K, name.encode())
            ev = against_model(r, [circ] * K, recs)
            assert ev["waves"] == 1 and ev["items_per_chunk"] == 2 and ev["chunks"] == (K + 1) // 2, ev
            seen.append(ev["items_per_chunk"])
        for K in (seen[0], seen[0] + 1):
            ev = against_model(r, [circ] * K, W.challenge_set("edges", circ.lgN, K, name.encode()))
            assert ev["count"] == K and ev["chunks"] == K, ev


# ------------------------------------------------------------------------------------------------ 6. per-item constants
def _weights_bytes(tmpl, z=sc(W.filler(b"weights z"))):
    return tmpl.test_weights(z)


@pytest.mark.parametrize("name,args,cap", [("inequality", NE_ARGS, 4), ("less_than", LT_ARGS, 512)], ids=["inequality", "less_than"])
def test_per_item_public_inputs(ctx, name, args, cap):
    """8 items against 8 different public values on ONE template: n = 3 (N = 4, the smallest) and N = 512"""
    S = Inputs(ctx, name, args)
    try:
        tmpl = S.tmpl
        assert len(args) == 8 and len(set(S.inputs)) == 8 and tmpl.n_inputs == len(S.inputs[0]) // 32 > 0
        before = _weights_bytes(tmpl)
        (st, states), counts = launches(ctx, lambda: tmpl.verify_batch(S.items(), batch_seed=BATCH_SEED))
        assert st == [0] * 8, st
        assert counts["k_bucket_chunks"] == 1 and counts["k_vw_tails"] == 1 and "k_input_slots" not in counts and "k_verify_scalars" not in counts, counts
        assert _weights_bytes(tmpl) == before, "an accepted call changed the circuit"
        # each state is what set_inputs + verify leaves; afterwards the standing slots are put back as they were
        # the hook's w_c per item is the model's over the host assembly with that item's values baked in
        recs = W.challenge_set("hashed", S.rows[0].N.bit_length() - 1, 8, name.encode())
        ev = against_model(tmpl, S.rows, recs, inputs=S.inputs)
        assert ev["n_tail"] > 0 and ev["launches"]["k_vw_tails"] == ev["waves"] == 1, ev
        assert len({s[-2] for s in W.wave_bytes(S.rows, recs)[2]}) == 8, "w_c does not depend on the public values: the case proves nothing"
        # item 5 given item 4's inputs: status 3 for item 5 alone (the rejected sum is judged item by item, constants written and put back)
        st, _ = tmpl.verify_batch(S.items(inputs={5: S.inputs[4]}), batch_seed=BATCH_SEED)
        assert st == [0] * 5 + [3] + [0] * 2, st
        assert _weights_bytes(tmpl) == before, "a rejected call changed the circuit"
        # an item that brings nothing is judged on the STANDING slots: wrong for it while another item's values stand, right once its own do
        tmpl.set_inputs([S.inputs[3][32 * j:32 * j + 32] for j in range(tmpl.n_inputs)])
        standing = _weights_bytes(tmpl)
        assert standing != before
        st, _ = tmpl.verify_batch(S.items(inputs={2: None, 3: None}), batch_seed=BATCH_SEED)
        assert st == [0, 0, 3, 0] + [0] * 4, st
        assert _weights_bytes(tmpl) == standing
        (st, _), counts = launches(ctx, lambda: tmpl.verify_batch(S.items(order=[3, 0, 3], inputs={3: None}), batch_seed=BATCH_SEED))
        assert st == [0, 0, 0] and counts["k_bucket_chunks"] == 1, (st, counts)
        # every status is bpg_r1cs_set_inputs + bpg_r1cs_verify_resident on the item alone
        for k in (0, 7):
            tmpl.set_inputs([S.inputs[k][32 * j:32 * j + 32] for j in range(tmpl.n_inputs)])
            assert alone(ctx, tmpl, S.state[k], S.coms[k], S.proofs[k], vseed(k), 0) == (0, states[k])
    finally:
        S.free()


def test_per_item_parameter_values(ctx):
    """a template with a parameter row (the root of an 8-leaf Merkle tree): four trees, four roots, one call"""
    from bulletproofs_gadgets_amd import workloads
    from test_template_gpu import constant_term, last_row
    trees = [workloads.merkle_full_tree(ctx, leaves=8, seed=s) for s in (2, 3, 4, 5)]
    ctx.gens_ensure(trees[0].gens_capacity)
    tmpl = trees[0].prover.template(ctx, param_rows=[last_row(trees[0])])
    try:
        insts = [t.prover.instance() for t in trees]
        params = [constant_term(i, last_row(t)) for i, t in zip(insts, trees)]
        assert len(set(params)) == 4 and tmpl.n_params == 1
        proofs = []
        for t, i, p in zip(trees, insts, params):
            tmpl.assign(i.v, [p])
            proofs.append(tmpl.prove(t.transcript.state, i.v_blinding, rng("vw param"))[0])
        before = _weights_bytes(tmpl)
        items = [(t.transcript.state, b"".join(t.commitments), pr, vseed(k), 0, p) for k, (t, pr, p) in enumerate(zip(trees, proofs, params))]
        (st, _), counts = launches(ctx, lambda: tmpl.verify_batch(items, batch_seed=BATCH_SEED))
        assert st == [0] * 4 and counts["k_bucket_chunks"] == 1 and counts["k_vw_tails"] == 1, (st, counts)
        swapped = [it[:5] + (params[(k + 1) % 4] if k == 2 else it[5],) for k, it in enumerate(items)]
        assert tmpl.verify_batch(swapped, batch_seed=BATCH_SEED)[0] == [0, 0, 3, 0]
        assert tmpl.verify_batch([it[:5] for it in items], batch_seed=BATCH_SEED)[0] == [3, 3, 3, 0]          # the standing root is the last assign's
        assert _weights_bytes(tmpl) == before
        rows = [W.Rows(i) for i in insts]
        recs = W.challenge_set("edges", rows[0].N.bit_length() - 1, 4, b"param")
        ev = against_model(tmpl, rows, recs, params=params)
        assert ev["n_tail"] == 1, ev
        # inputs on a circuit without inputs, constants on a repeat: refused, nothing launched
        rep = tmpl.repeat(2)
        plain = ctx.upload(insts[0])                                              # a plain upload has no parameter rows
        try:
            ctx.profile_set(2)
            for c, it in ((tmpl, items[0][:6] + (bytes(32),)), (rep, (bytes(203), bytes(32 * rep.m), bytes(64), vseed(0), 0, params[0] + params[1]))):
                with pytest.raises(bpg.BpgError) as e:
                    c.verify_batch([it], batch_seed=BATCH_SEED)
                assert e.value.status == 4 and "item 0" in str(e.value), str(e.value)
            with pytest.raises(bpg.BpgError) as e:
                plain.verify_batch([items[0]], batch_seed=BATCH_SEED)
            assert e.value.status == 4 and "item 0" in str(e.value), str(e.value)
            assert ctx.profile_report() == {}
        finally:
            ctx.profile_set(0)
            rep.free(); plain.free()
    finally:
        tmpl.free()


# ------------------------------------------------------------------------------------------------ 7. standing constants on a repeat and on a join
def test_standing_constants_on_a_repeat_and_on_a_join():
    from test_template_repeat_gpu import host, template, SEED
    from test_template_join_gpu import host as join_host
    ctx = bpg.Context(0)
    try:
        ctx.gens_ensure(64)
        tmpls = {name: template(ctx, name) for name in ("set3", "bounds8")}
        rep, joined = tmpls["set3"].repeat(2), ctx.join([(tmpls["set3"], 1), (tmpls["bounds8"], 1)])
        for c, h in ((rep, host(ctx, "set3", "vw-rep", 2)), (joined, join_host(ctx, [("set3", 1), ("bounds8", 1)], "vw-join"))):
            assert (c.n, c.m) == (h.inst.n, h.inst.m) and c.n <= 64
            c.assign(h.inst.v, h.params)
            proofs = [c.prove(h.state, h.inst.v_blinding, hashlib.sha256(SEED + bytes([k])).digest())[0] for k in range(4)]
            assert len(set(proofs)) == 4
            items = [(h.state, h.coms, p, vseed(k), 0) for k, p in enumerate(proofs)]
            (st, _), counts = launches(ctx, lambda: c.verify_batch(items, batch_seed=BATCH_SEED))
            assert st == [0] * 4 and counts["k_bucket_chunks"] == 1 and "k_vw_tails" not in counts and counts["k_vw_scalars"] == 1, (st, counts)
            bad = proofs[1][:-1] + bytes([proofs[1][-1] ^ 1])                     # b of the inner-product argument
            st, _ = c.verify_batch(items[:1] + [(h.state, h.coms, bad, vseed(1), 0)] + items[2:], batch_seed=BATCH_SEED)
            assert st == [0, 3, 0, 0]
        for c in [rep, joined] + list(tmpls.values()):
            c.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. refused calls touch nothing
def test_refused_calls_touch_nothing(ctx, corpus):
    circs, by_circuit, _, res = corpus
    b = by_circuit["small5"][0]
    r = res["small5"]
    lib = bpg.lib()
    other = bpg.Context(0)
    try:
        other.gens_ensure(8)
        foreign = other.upload(b.circuit)
        state = C.create_string_buffer(bytes(b.state), 203)

        def item(**null):
            it = bpg.VerifyResidentItem()
            it.transcript_state = C.cast(state, C.c_void_p); it.V = b.V; it.proof = b.proof; it.proof_len = len(b.proof); it.seed = b.seed; it.flags = b.flags
            for k in null:
                setattr(it, k, None)
            return it

        status = (C.c_int32 * 2)(77, 77)
        ctx.profile_set(2); other.profile_set(2)
        calls = [("another context", ctx._h, foreign._h, (item(), item()), status),
                 ("another context", other._h, r._h, (item(), item()), status),
                 ("null circuit", ctx._h, None, (item(), item()), status),
                 ("null items", ctx._h, r._h, None, status),
                 ("null items", ctx._h, r._h, (item(), item()), None),
                 ("ctx", None, r._h, (item(), item()), status)]
        calls += [("item 1: null " + f, ctx._h, r._h, (item(), item(**{f: True})), status) for f in ("transcript_state", "proof", "seed", "V")]
        for word, c, h, items, st in calls:
            arr = (bpg.VerifyResidentItem * 2)(*items) if items else None
            rc = lib.bpg_r1cs_verify_resident_batch(c, h, C.c_uint64(2), arr, BATCH_SEED, st)
            assert rc == 4 and word in lib.bpg_last_error().decode(), (word, rc, lib.bpg_last_error())
            assert list(status) == [77, 77] and state.raw[:203] == bytes(b.state), word
        # the hook's refusals: a non-canonical entry, y^-1 = 0, a u_k = 0, a u_k^-1 that is not the inverse, no item
        good = W.challenge_set("hashed", 3, 2)
        for change in ({"yinv": 0}, {"z": W.L}, {"uk": [0, 1, 1], "ukinv": [0, 1, 1]}, {"ukinv": [1, 1, 1]}, {"rho": 2**256 - 1}):
            with pytest.raises(bpg.BpgError) as e:
                hook(r, [good[0], dict(good[1], **change)])
            assert e.value.status == 4 and "item 1" in str(e.value), str(e.value)
        with pytest.raises(bpg.BpgError):
            hook(r, [])
        assert ctx.profile_report() == {} and other.profile_report() == {}, "a refused call launched"
        foreign.free()
    finally:
        ctx.profile_set(0)
        other.close()


# ------------------------------------------------------------------------------------------------ 9. nothing leaks
def test_nothing_leaks():
    """a process of its own: an accepted call, a rejected call with per-item constants (the item-by-item pass and its buffers) and the hook; after the context
    closes the census is all zero"""
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "leak"], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["ok"] is True
    assert any(got["open"]) and got["end"] == [0] * 6, got
