"""The GPU verifier against the malformed-proof corpus of tests/verify_cases.py: every record through bpg_r1cs_verify (Context.verify_flat's call)
and bpg_r1cs_verify_resident, a mutant of every (field kind x class) through bpg_r1cs_verify_batch among good neighbours, and the device decoder
(k_decompress through bpg_test_decompress) against pyref.decompress.  The status must be the CPU oracle's status exactly.

Transcript state after the call.  An accepted proof leaves the oracle's state.  After a REJECTION equality with the oracle is not demanded: the
oracle returns early without writing its transcript back (format and identity errors), upstream consumes the transcript either way, and no caller
can use the state of a refused proof; what is demanded is that the flat, resident and batch paths leave the SAME state as each other, so that
bpg_r1cs_verify_batch stays "what the call alone leaves" (include/bpg.h).

Every input is data the verifier has to refuse on its ordinary path; the hook validates its arguments on the host."""
import collections
import ctypes as C
import hashlib
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import verify_cases as VC

pytestmark = pytest.mark.gpu
BATCH_SEEDS = (bytes(32), hashlib.sha256(b"malformed batch").digest())
GOOD = ("small5/f0", "one/f1", "none/f2", "range8/f3", "range56/f0", "big/f1", "small5/f2", "range56/f3")


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    circs, bases, mutants = VC.corpus()
    gens = O.Gens(1024)
    accepted = {}
    for r in bases:
        rc, state = VC.oracle_verify(gens, r.state, r.circuit, r.V, r.proof, r.seed, r.flags)
        assert rc == 0
        accepted[r.name] = state
    return circs, bases, mutants, accepted


def verify_flat(ctx, r):
    """bpg_r1cs_verify -> (status, transcript state after)"""
    ts = C.create_string_buffer(bytes(r.state), 203)
    cs = r.circuit.cstruct()
    s = bpg.lib().bpg_r1cs_verify(ctx._h, C.byref(cs), ts, C.c_uint64(r.circuit.m), r.V, r.proof, C.c_uint64(len(r.proof)), r.seed, C.c_uint32(r.flags))
    return s, ts.raw[:203]


def verify_resident(ctx, res, r):
    """bpg_r1cs_verify_resident -> (status, transcript state after)"""
    ts = C.create_string_buffer(bytes(r.state), 203)
    s = bpg.lib().bpg_r1cs_verify_resident(ctx._h, res._h, ts, C.c_uint64(res.m), r.V, r.proof, C.c_uint64(len(r.proof)), r.seed, C.c_uint32(r.flags))
    return s, ts.raw[:203]


def both_paths(ctx, records, shared):
    """every record through the flat and the resident entry point -> {name: (status, state)} (asserted equal between the two)"""
    out = {}
    for r in records:
        res = shared.get(id(r.circuit)) or ctx.upload(r.circuit)
        try:
            flat, resident = verify_flat(ctx, r), verify_resident(ctx, res, r)
        finally:
            if id(r.circuit) not in shared:
                res.free()
        assert flat[0] == resident[0] == r.status, (r.name, flat[0], resident[0], r.status)
        assert flat[1] == resident[1], r.name
        out[r.name] = flat
    return out


@pytest.fixture(scope="module")
def single(ctx, corpus):
    """the single-proof matrix: every record the main context can take (its capacity covers every circuit), on both entry points"""
    _, bases, mutants, accepted = corpus
    shared = {id(r.circuit): ctx.upload(r.circuit) for r in bases}
    recs = [r for r in bases + mutants if r.cls != "capacity"]
    out = both_paths(ctx, recs, shared)
    for res in shared.values():
        res.free()
    print("verify corpus on the GPU: %d records through bpg_r1cs_verify, %d through bpg_r1cs_verify_resident" % (len(out), len(out)))
    return out


def test_every_record_on_the_flat_and_the_resident_path(ctx, corpus, single):
    _, bases, mutants, accepted = corpus
    n_cap = sum(r.cls == "capacity" for r in mutants)
    assert len(single) == len(bases) + len(mutants) - n_cap
    for r in bases:
        assert single[r.name] == (0, accepted[r.name]), r.name             # accepted: the oracle's transcript state
    assert all(single[r.name][0] == r.status != 0 for r in mutants if r.cls != "capacity")


def test_capacity_below_N_on_all_three_paths(corpus):
    """a context whose generator table is shorter than the padded circuit: INVALID_GENERATORS_LENGTH for that item alone"""
    _, bases, mutants, accepted = corpus
    by_base = {r.name: r for r in bases}
    caps = sorted({r.capacity for r in mutants if r.cls == "capacity"})
    assert caps == [4, 512]
    total = 0
    for cap in caps:
        c2 = bpg.Context(0)
        try:
            c2.gens_ensure(cap)
            recs = [r for r in mutants if r.cls == "capacity" and r.capacity == cap]
            alone = both_paths(c2, recs, {})
            assert all(s == (1, r.state) for r, s in ((r, alone[r.name]) for r in recs))          # refused before the transcript is touched
            good = [by_base[n] for n in ("one/f0", "none/f3", "one/f2")]                                # N = 1: within any capacity
            for seed in BATCH_SEEDS:
                items = [(r.circuit, r.state, r.V, r.proof, r.seed, r.flags) for r in good[:2] + recs + good[2:]]
                st, states = c2.verify_batch(items, batch_seed=seed)
                assert st == [0, 0] + [1] * len(recs) + [0]
                assert states == [accepted[g.name] for g in good[:2]] + [r.state for r in recs] + [accepted[good[2].name]]
            total += len(recs)
        finally:
            c2.close()
    assert total == sum(r.cls == "capacity" for r in mutants)
    print("capacity mutants: %d through each of the three entry points" % total)


def pick_mutants(mutants):
    """one mutant per (field kind x class), walking through the bases so that circuits, N and dialects vary"""
    cells = collections.OrderedDict()
    for r in mutants:
        if r.cls != "capacity":
            cells.setdefault((r.kind, r.cls), []).append(r)
    return [c[(7 * k) % len(c)] for k, c in enumerate(cells.values())]


def run_batch(ctx, recs, uploads, seed):
    items = [(uploads.get(r.name, r.circuit), r.state, r.V, r.proof, r.seed, r.flags) for r in recs]
    return ctx.verify_batch(items, batch_seed=seed)


def test_the_good_items_alone_are_accepted_by_the_one_msm(ctx, corpus):
    """the eight neighbours of the placements below - padded circuits (5 -> 8, 56 -> 64, 700 -> 1024), N = 1, commitments - are accepted by the
    weighted sum itself: one MSM, no item-by-item pass behind which a wrong accumulator (a lost padding factor u, say) could hide"""
    _, bases, _, accepted = corpus
    by_base = {r.name: r for r in bases}
    good = [by_base[n] for n in GOOD]
    for seed in BATCH_SEEDS:
        ctx.profile_set(1)
        st, states = run_batch(ctx, good, {}, seed)
        rep = ctx.profile_report()
        ctx.profile_set(0)
        assert st == [0] * 8 and states == [accepted[g.name] for g in good]
        assert rep["k_bucket_chunks"]["count"] == 1


def test_one_mutant_among_eight_good_items(ctx, corpus, single):
    """first, in the middle and last among eight good items of four circuits, N = 1 .. 1024, flat and resident, some with commitments: the mutant's status is
    its status alone and every neighbour's is 0; states as the calls alone leave them"""
    _, bases, mutants, accepted = corpus
    by_base = {r.name: r for r in bases}
    good = [by_base[n] for n in GOOD]
    assert len({g.base.split("/")[0] for g in good}) >= 3 and len({g.circuit.n for g in good}) >= 2 and any(g.circuit.m for g in good)
    uploads = {"big/f1": ctx.upload(by_base["big/f1"].circuit)}                 # a resident item among flat ones
    picked = pick_mutants(mutants)
    want_cells = {(r.kind, r.cls) for r in mutants if r.cls != "capacity"}
    assert {(r.kind, r.cls) for r in picked} == want_cells and len(picked) == len(want_cells) >= 6 * 8 - 2 + 5 * 7 + 8 + 9
    assert len({r.base for r in picked}) >= 12 and len({r.circuit.n for r in picked}) >= 5
    batches = 0
    for bad in picked:
        for pos in (0, 4, 8):
            recs = good[:pos] + [bad] + good[pos:]
            for seed in BATCH_SEEDS:
                st, states = run_batch(ctx, recs, uploads, seed)
                assert st == [0] * pos + [bad.status] + [0] * (8 - pos), (bad.name, pos, st)
                assert states == [accepted[g.name] for g in good[:pos]] + [single[bad.name][1]] + [accepted[g.name] for g in good[pos:]], (bad.name, pos)
                batches += 1
    uploads["big/f1"].free()
    print("batch placements: %d mutants x 3 positions x 2 batch seeds = %d batches of 9 through bpg_r1cs_verify_batch" % (len(picked), batches))


def test_batches_of_mutants_only_and_of_mixed_sizes(ctx, corpus, single):
    _, bases, mutants, accepted = corpus
    by_name = {r.name: r for r in bases + mutants}
    picked = pick_mutants(mutants)
    # every item a mutant (nothing to accept: every status its own)
    for seed in BATCH_SEEDS:
        st, states = run_batch(ctx, picked, {}, seed)
        assert st == [r.status for r in picked]
        assert states == [single[r.name][1] for r in picked]
    # two mutants of different N that both reach the one MSM, among good items
    pair = [by_name["big/f0/a=plus_1"], by_name["small5/f2/R_1=other_point"]]
    assert pair[0].circuit.n != pair[1].circuit.n
    good = [by_name[n] for n in GOOD]
    recs = good[:3] + [pair[0]] + good[3:6] + [pair[1]] + good[6:]
    for seed in BATCH_SEEDS:
        st, states = run_batch(ctx, recs, {}, seed)
        assert st == [0, 0, 0, 3, 0, 0, 0, 3, 0, 0]
        assert states == [single[r.name][1] if r.status else accepted[r.name] for r in recs]
    # the largest-N item is the bad one: the accumulators past every good item's N hold its terms alone
    small_good = [g for g in good if g.circuit.n <= 56] + [by_name["range8/f0"]]
    assert max(g.circuit.n for g in small_good) == 56
    for name in ("big/f0/a=plus_1", "big/f1/L_3=other_point", "big/f2/coef-left@699", "big/f3/coef-right@512", "big/f0/V_2=other_point", "big/f2/replace-V_1",
                 "big/f1/b=minus_1", "big/f3/T_4=negation", "big/f0/coef-output@256"):
        bad = by_name[name]
        for pos in (0, len(small_good)):
            recs = small_good[:pos] + [bad] + small_good[pos:]
            for seed in BATCH_SEEDS:
                st, states = run_batch(ctx, recs, {}, seed)
                assert st == [0] * pos + [3] + [0] * (len(small_good) - pos), (name, pos, st)
                assert states[pos] == single[name][1]


def test_weights_defeat_a_cancelling_pair_with_commitments(ctx, corpus, single):
    """a is never absorbed into the transcript: copies with a + 1 and a - 1 see the same challenges and their residuals are +Q and -Q - on circuits
    whose weighted sum holds V terms (m = 2 and m = 3)"""
    _, bases, mutants, accepted = corpus
    by_name = {r.name: r for r in bases + mutants}
    for base in ("small5/f0", "small5/f3", "big/f1", "big/f2", "one/f0"):
        recs = [by_name[base + "/a=plus_1"], by_name[base + "/a=minus_1"], by_name[base]]
        assert recs[2].circuit.m > 0
        for seed in BATCH_SEEDS:
            st, _ = run_batch(ctx, recs, {}, seed)
            assert st == [3, 3, 0], base


def test_device_decoder_matches_the_python_reference(ctx, golden):
    """k_decompress on the vectors of the host build (tests/test_verify_malformed_host.py): decision, x, y and re-encoding against pyref.decompress"""
    vectors = VC.decoder_vectors(golden)
    counts = VC.check_decoder(ctx.test_decompress, vectors)
    VC.check_decoder_counts(counts)
    assert ctx.test_decompress([]) == ([], [])
    lib = bpg.lib()
    ctx.profile_set(2)
    assert lib.bpg_test_decompress(ctx._h, C.c_uint64(2), None, (C.c_uint32 * 2)(), C.create_string_buffer(128)) == 4
    assert lib.bpg_test_decompress(ctx._h, C.c_uint64(2), bytes(64), None, C.create_string_buffer(128)) == 4
    assert lib.bpg_test_decompress(ctx._h, C.c_uint64(2), bytes(64), (C.c_uint32 * 2)(), None) == 4
    assert lib.bpg_test_decompress(ctx._h, C.c_uint64((1 << 24) + 1), bytes(64), (C.c_uint32 * 2)(), C.create_string_buffer(128)) == 4
    assert ctx.profile_report() == {}                                     # refused on the host: no launch
    ctx.profile_set(0)
    print("decoder vectors on the GPU: %d %s" % (len(vectors), dict(counts)))
