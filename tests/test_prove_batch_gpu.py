"""Lockstep batch proving on the GPU (bpg_r1cs_prove_batch, Context.prove_batch): every item's proof, transcript state and status are exactly what
bpg_r1cs_prove gives for it alone, while the small items of a wave share every launch."""
import ctypes as C
import hashlib
import json
import os
import pathlib
import random
import subprocess
import sys
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import gen_proof_fixtures as G
import gen_big_proof_fixtures as GB
import assembly_cases as AC

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
FIX = json.loads((ROOT / "tests" / "golden" / "proofs.json").read_text())["proofs"]
BIG = json.loads((ROOT / "tests" / "golden" / "proofs_big.json").read_text())["proofs"]
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(1 << 16)
    yield c
    c.close()


def _alone(ctx, item):
    """bpg_r1cs_prove of one item: (status, proof or None, transcript state after)"""
    arr, keep = bpg._batch_items([item])
    it = arr[0]
    s = bpg.lib().bpg_r1cs_prove(ctx._h, it.inst, C.c_void_p(it.transcript_state), C.c_uint64(it.m), item[2], item[3], C.c_uint32(it.flags),
                                 C.c_void_p(it.proof_out), it.proof_len)
    k = keep[0]
    return s, (k[2].raw[:k[3].value] if s == 0 else None), k[1].raw[:203]


def _fixture_items():
    built = {name: G.build(name) for name in sorted({r["circuit"] for r in FIX})}
    return [(built[r["circuit"]][0], built[r["circuit"]][1], b"", bytes.fromhex(r["seed"]), r["flags"]) for r in FIX]


def _rand_circuit(n, seed, satisfied=True):
    """n multipliers with random inputs, m = 0, and a linear constraint per multiplier pinning its left input (one of them wrong if not satisfied)"""
    rnd = random.Random(seed)
    t = bpg.Transcript(b"RandomCircuit")
    p = bpg.Prover(None, t)
    one = (1).to_bytes(32, "little")
    for i in range(n):
        a, b = rnd.randrange(bpg.L), rnd.randrange(bpg.L)
        l, r, o = p.allocate_multiplier((a.to_bytes(32, "little"), b.to_bytes(32, "little")))
        want = a if (satisfied or i != 0) else (a + 1) % bpg.L
        if i % 3 != 2:
            p.constrain(bpg.LinearCombination([(l, one), (bpg.Variable.One(), ((bpg.L - want) % bpg.L).to_bytes(32, "little"))]))
    return p.instance(), t.state


def _cfg2(ctx, k):
    a = workloads.bounds_check_64(ctx, seed=k)
    inst = a.prover.instance()
    return (inst, a.transcript.state, inst.v_blinding, hashlib.sha256(b"cfg2 %d" % k).digest(), k % 4), b"".join(a.commitments)


def test_all_fixtures_in_one_call(ctx):
    items = _fixture_items()
    res, st = ctx.prove_batch(items, return_status=True)
    assert st == [0] * 35
    for (proof, state), r, it in zip(res, FIX, items):
        assert hashlib.sha256(proof).hexdigest() == r["sha256"]
        if "proof" in r:
            assert proof.hex() == r["proof"]
        assert (0, proof, state) == _alone(ctx, it)


def test_mixed_batch_with_a_fallback_item(ctx):
    items, circuits = [], []
    for name in ("bounds_check_reference", "cfg2_bounds_check_64", "mimc_1_block", "mimc_3_blocks", "merkle_4"):
        p, t, coms = AC.build(bpg, name, ctx)
        inst = p.instance()
        items.append((inst, t.state, inst.v_blinding, hashlib.sha256(name.encode()).digest(), len(items) % 4))
        circuits.append((inst, t.state, b"".join(coms)))
    for n, seed in ((1, 1), (5, 2), (300, 3), (1024, 4)):
        inst, state = _rand_circuit(n, seed)
        items.append((inst, state, b"", bytes([seed]) * 32, seed % 4))
        circuits.append((inst, state, b""))
    a3 = GB.build("cfg3_mimc67", ctx)                                   # N = 2^16: above the lockstep limit
    inst3 = a3.prover.instance()
    rec3 = next(r for r in BIG if r["circuit"] == "cfg3_mimc67" and r["flags"] == 0)
    items.append((inst3, a3.transcript.state, inst3.v_blinding, bytes.fromhex(rec3["seed"]), 0))
    res = ctx.prove_batch(items)
    assert hashlib.sha256(res[-1][0]).hexdigest() == rec3["sha256"]
    for k, it in enumerate(items):
        assert (0,) + res[k] == _alone(ctx, it), k
    og = O.Gens(8192)
    for k, (inst, state, coms) in enumerate(circuits):
        assert O.verify(og, state, G.to_oracle(inst), coms, res[k][0], SEED, items[k][4]) == 0, k


def test_many_cfg2_items_in_one_call(ctx):
    pairs = [_cfg2(ctx, k) for k in range(1024)]
    items = [p[0] for p in pairs]
    res = ctx.prove_batch(items)
    vitems = [(it[0], it[1], coms, proof, SEED, it[4] & 3) for (it, coms), (proof, _) in zip(pairs, res)]
    st, _ = ctx.verify_batch(vitems, batch_seed=bytes(32))
    assert st == [0] * 1024
    assert len({proof for proof, _ in res}) == 1024
    for k in range(0, 1024, 32):
        assert (0,) + res[k] == _alone(ctx, items[k]), k


def test_order_duplicates_and_an_unsatisfied_witness(ctx):
    items = [_cfg2(ctx, k)[0] for k in range(6)]
    bad_inst, bad_state = _rand_circuit(64, 9, satisfied=False)
    items.insert(3, (bad_inst, bad_state, b"", SEED, 0))
    res = ctx.prove_batch(items)
    perm = [6, 0, 3, 5, 1, 4, 2]
    res_p = ctx.prove_batch([items[i] for i in perm])
    assert [res[i] for i in perm] == res_p
    dup = ctx.prove_batch([items[2], items[2]])
    assert dup == [res[2], res[2]]
    assert (0,) + res[3] == _alone(ctx, items[3])
    assert O.verify(O.Gens(64), bad_state, G.to_oracle(bad_inst), b"", res[3][0], SEED, 0) != 0
    good_inst, good_state = _rand_circuit(64, 9)
    assert O.verify(O.Gens(64), good_state, G.to_oracle(good_inst), b"", ctx.prove_flat(good_inst, good_state, b"", SEED, 0)[0], SEED, 0) == 0


def test_failures_stay_with_their_item(ctx):
    items = [_cfg2(ctx, k)[0] for k in range(6)]
    lib = bpg.lib()

    def run(mutate):
        arr, keep = bpg._batch_items(items)
        mutate(arr, keep)
        status = (C.c_int32 * len(items))(*([77] * len(items)))
        rc = lib.bpg_r1cs_prove_batch(ctx._h, C.c_uint64(len(items)), arr, status)
        return rc, list(status), arr, keep

    def null_out(arr, keep): arr[1].proof_out = None
    def short(arr, keep): keep[2][3].value = 100
    def bad_csr(arr, keep): keep[4][0].nnz += 1
    rc, st, arr, keep = run(lambda a, k: (null_out(a, k), short(a, k), bad_csr(a, k)))
    assert st == [0, 4, 4, 0, 4, 0] and rc == 4
    assert "item 1" in lib.bpg_last_error().decode()
    for k in (0, 3, 5):
        assert (0, keep[k][2].raw[:keep[k][3].value], keep[k][1].raw[:203]) == _alone(ctx, items[k])
    for k in (1, 2, 4):                                                 # untouched transcript state, as bpg_r1cs_prove leaves it
        assert keep[k][1].raw[:203] == bytes(items[k][1])
    # the same items through bpg_r1cs_prove, one by one: the same statuses
    arr, keep = bpg._batch_items(items)
    null_out(arr, keep); short(arr, keep); bad_csr(arr, keep)
    for k in range(len(items)):
        it = arr[k]
        assert lib.bpg_r1cs_prove(ctx._h, it.inst, C.c_void_p(it.transcript_state), C.c_uint64(it.m), items[k][2], items[k][3], C.c_uint32(it.flags),
                                  C.c_void_p(it.proof_out), it.proof_len) == st[k]
    # a generator capacity below N fails that item alone
    c2 = bpg.Context(0)
    try:
        c2.gens_ensure(128)
        merkle = next(it for it in _fixture_items() if it[0].n > 128)
        mixed = [items[0], merkle, items[1]]
        res, st = c2.prove_batch(mixed, return_status=True)
        assert st == [0, 1, 0] and res[1][0] is None
        assert res[0] == _alone(ctx, items[0])[1:] and res[2] == _alone(ctx, items[1])[1:]
    finally:
        c2.close()


def _verify(ctx, inst, state, coms, proof, flags):
    """bpg_r1cs_verify from the state before the proof: (status, transcript state after)"""
    ts = C.create_string_buffer(bytes(state), 203)
    cs = inst.cstruct()
    cs.aL = cs.aR = cs.aO = None
    s = bpg.lib().bpg_r1cs_verify(ctx._h, C.byref(cs), ts, C.c_uint64(inst.m), bytes(coms), bytes(proof), C.c_uint64(len(proof)), SEED, C.c_uint32(flags))
    return s, ts.raw[:203]


def test_prover_and_verifier_share_one_script_at_its_edges(ctx):
    """The transcript steps that prove(), prove_batch() and the verifier share, where they can go wrong: n = 1 (lg N = 0: no inner-product round), n = 2,
    n = 3 (padded to N = 4), the range8 fixture and a 64-bit bounds check (m > 0: commitments, t_x_blinding takes <w_V, v_blinding>), each under flags
    0..3, all in ONE call.  Every item: the bytes and the final transcript state of bpg_r1cs_prove for it alone; bpg_r1cs_verify accepts it from the
    state before the proof and leaves the PROVER's final state.  What this guards: the code AROUND the shared steps (which step each path calls when,
    the `if lg N` branches, padding, the proof-byte layout, the tb[2] sum) at shapes other tests reach by accident.  What it cannot catch: a wrong label or
    a wrong order INSIDE a shared step - all three roles would follow it together.  The reference's recorded proofs guard that (test_proof_fixtures.py,
    test_gpu_parity.py, test_all_fixtures_in_one_call above)."""
    circuits = [_rand_circuit(n, 40 + n) + (b"", b"") for n in (1, 2, 3)]
    r8, r8_state, _ = G.build("range8")
    circuits.append((r8, r8_state, r8.v_blinding, b""))
    (c2, c2_state, c2_vb, _, _), c2_coms = _cfg2(ctx, 7)
    circuits.append((c2, c2_state, c2_vb, c2_coms))
    assert [c[0].n for c in circuits[:3]] == [1, 2, 3] and circuits[3][0].n == 8 and circuits[4][0].m > 0
    items = [(inst, state, vb, hashlib.sha256(b"edge %d %d" % (k, fl)).digest(), fl) for k, (inst, state, vb, _) in enumerate(circuits) for fl in range(4)]
    res, st = ctx.prove_batch(items, return_status=True)
    assert st == [0] * len(items)
    for k, (it, (proof, state)) in enumerate(zip(items, res)):
        assert (0, proof, state) == _alone(ctx, it), k
        assert len(proof) == (353 if it[4] & 1 else 448) + 64 * max(it[0].n - 1, 0).bit_length() + 64, k
        assert _verify(ctx, it[0], it[1], circuits[k // 4][3], proof, it[4]) == (0, state), k


def _launches(ctx, items):
    ctx.profile_set(2)
    ctx.prove_batch(items)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    return sum(v["count"] for v in rep.values())


def test_lockstep_launch_count_does_not_grow_with_the_batch(ctx):
    items = [_cfg2(ctx, k)[0] for k in range(256)]
    ctx.prove_batch(items[:8])                                          # warm: window tables of N = 128 built
    l8, l256 = _launches(ctx, items[:8]), _launches(ctx, items)
    ctx.profile_set(2)
    for it in items[:8]:
        _alone(ctx, it)
    single = sum(v["count"] for v in ctx.profile_report().values())
    ctx.profile_set(0)
    assert l8 == l256 < single, (l8, l256, single)


KNOB_SCRIPT = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/tests/golden")
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import gen_proof_fixtures as G
ctx = bpg.Context(0)
ctx.gens_ensure(8192)
items = []
for k in range(5):
    a = workloads.bounds_check_64(ctx, seed=k)
    inst = a.prover.instance()
    items.append((inst, a.transcript.state, inst.v_blinding, hashlib.sha256(b"cfg2 %d" % k).digest(), k % 4))
inst, state, _ = G.build("merkle4")
items.append((inst, state, b"", bytes(32), 1))
print(json.dumps([[p.hex(), s.hex()] for p, s in ctx.prove_batch(items)]))
ctx.close()
"""


@pytest.mark.parametrize("env", [{"BPG_TT_ORIG_LG": "0"}, {"BPG_BATCH_WAVE_MB": "0"}, {"BPG_PROFILE": "serving"}])
def test_knobs_keep_the_bytes(ctx, env):
    items = [_cfg2(ctx, k)[0] for k in range(5)]
    inst, state, _ = G.build("merkle4")
    items.append((inst, state, b"", bytes(32), 1))
    want = [[p.hex(), s.hex()] for _, p, s in (_alone(ctx, it) for it in items)]
    r = subprocess.run([sys.executable, "-c", KNOB_SCRIPT, str(ROOT)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == want
