"""Batch verification on the GPU (bpg_r1cs_verify_batch, Context.verify_batch, `bpg_verifier --batch FILE --combine`): many proofs in ONE weighted
multiscalar multiplication, every status exactly what verifying the item alone gives."""
import ctypes as C
import hashlib
import json
import os
import pathlib
import shutil
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import build as bpg_build
import oracle_lib as O
import gen_proof_fixtures as G
import gen_big_proof_fixtures as GB

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
FIX = json.loads((ROOT / "tests" / "golden" / "proofs.json").read_text())["proofs"]
BIG = json.loads((ROOT / "tests" / "golden" / "proofs_big.json").read_text())["proofs"]
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    """the 35 fixture proofs (range8, range56, merkle4): (circuit, instance, state, proof, verifier flags); the 5 without recorded bytes are proved here"""
    built = {name: G.build(name) for name in sorted({r["circuit"] for r in FIX})}
    ctx.gens_ensure(max(cap for _, _, cap in built.values()))
    out = []
    for r in FIX:
        inst, state, _ = built[r["circuit"]]
        if "proof" in r:
            proof = bytes.fromhex(r["proof"])
        else:
            proof, _ = ctx.prove_flat(inst, state, b"", bytes.fromhex(r["seed"]), r["flags"])
        assert hashlib.sha256(proof).hexdigest() == r["sha256"]
        out.append((r["circuit"], inst, state, proof, r["flags"] & 3))
    assert len(out) == 35 and sum("proof" not in r for r in FIX) == 5
    return out


def _items(small, seed=SEED):
    return [(inst, state, b"", proof, seed, fl) for _, inst, state, proof, fl in small]


def _verify_alone(ctx, inst, state, coms, proof, seed, flags):
    """bpg_r1cs_verify of one item: (status, transcript state after)"""
    ts = C.create_string_buffer(bytes(state), 203)
    cs = inst.cstruct()
    cs.aL = cs.aR = cs.aO = None
    s = bpg.lib().bpg_r1cs_verify(ctx._h, C.byref(cs), ts, C.c_uint64(inst.m), bytes(coms), bytes(proof), C.c_uint64(len(proof)), seed, C.c_uint32(flags))
    return s, ts.raw[:203]


def test_all_small_fixtures_in_one_batch(ctx, small):
    ctx.profile_set(1)
    rc, st, _ = ctx.verify_batch(_items(small), batch_seed=bytes(32), return_status=True)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    assert rc == 0 and st == [0] * 35
    assert rep["k_bucket_chunks"]["count"] == 1                    # one MSM for 35 proofs of three circuits in four dialects


def test_bad_items_are_named_exactly(ctx, small):
    items = _items(small)
    r56 = [k for k, s in enumerate(small) if s[0] == "range56"]
    r8 = [k for k, s in enumerate(small) if s[0] == "range8"]
    a, b, c, d = r56[0], r56[4], r56[7], [k for k, s in enumerate(small) if s[0] == "merkle4"][1]
    inst, state, coms, proof, seed, fl = items[a]
    bad = bytearray(proof); bad[40] ^= 1                             # inside A_I1 / A_O1
    items[a] = (inst, state, coms, bytes(bad), seed, fl)
    inst, state, coms, proof, seed, fl = items[b]
    items[b] = (inst, state, coms, proof[:-1], seed, fl)             # truncated
    inst, state, coms, _, seed, _ = items[c]
    items[c] = (inst, state, coms, small[r8[0]][3], seed, small[r8[0]][4])      # a range8 proof in a range56 slot
    inst, _, coms, proof, seed, fl = items[d]
    items[d] = (inst, bpg.Transcript(b"AnotherLabel").state, coms, proof, seed, fl)      # valid proof, transcript of another label
    rc, st, states = ctx.verify_batch(items, batch_seed=bytes(32), return_status=True)
    og = O.Gens(8192)
    for k, (inst, state, coms, proof, seed, fl) in enumerate(items):
        alone, st_alone = _verify_alone(ctx, inst, state, coms, proof, seed, fl)
        assert st[k] == alone and states[k] == st_alone, k
        assert (st[k] != 0) == (O.verify(og, state, G.to_oracle(inst), b"", proof, seed, fl) != 0), k
    badset = {a, b, c, d}
    assert all(st[k] != 0 for k in badset) and all(st[k] == 0 for k in range(35) if k not in badset)
    assert st[b] == 2 and st[c] == 2
    assert rc == st[min(badset)]


def test_weights_defeat_a_cancelling_pair(ctx, small):
    """a is never absorbed into the transcript: copies with a + 1 and a - 1 see the same challenges, their residuals are +Q and -Q, and an
    unweighted sum would accept the pair"""
    _, inst, state, proof, fl = next(s for s in small if s[0] == "range56")
    n = len(proof)
    a = int.from_bytes(proof[n - 64:n - 32], "little")
    plus = proof[:n - 64] + ((a + 1) % bpg.L).to_bytes(32, "little") + proof[n - 32:]
    minus = proof[:n - 64] + ((a - 1) % bpg.L).to_bytes(32, "little") + proof[n - 32:]
    items = [(inst, state, b"", plus, SEED, fl), (inst, state, b"", minus, SEED, fl), (inst, state, b"", proof, SEED, fl)]
    st, _ = ctx.verify_batch(items, batch_seed=bytes(32))
    assert st == [3, 3, 0]


def test_transcript_states_and_batch_seeds(ctx, small):
    items = _items(small)[:12]
    st, states = ctx.verify_batch(items, batch_seed=b"\x01" * 32)
    assert st == [0] * 12
    for k, it in enumerate(items):
        assert (0, states[k]) == _verify_alone(ctx, *it)
    assert ctx.verify_batch(items, batch_seed=b"\x01" * 32) == (st, states)             # same batch seed, same outcome
    for s in (b"\x02" * 32, b"\x03" * 32, None):
        assert ctx.verify_batch(items, batch_seed=s)[0] == [0] * 12


def test_refused_arguments_touch_nothing(ctx, small):
    _, inst, state, proof, fl = small[0]
    res = ctx.upload(inst)
    lib = bpg.lib()
    for case in ("both", "wrong m", "neither"):
        arr, states, keep = bpg._verify_items([(inst, state, b"", proof, SEED, fl), (inst, state, b"", proof, SEED, fl)])
        if case == "both":
            arr[1].circuit = res._h
        elif case == "wrong m":
            arr[1].m = 1; arr[1].V = bytes(32)
        else:
            arr[1].inst = None
        status = (C.c_int32 * 2)(77, 77)
        ctx.profile_set(2)
        rc = lib.bpg_r1cs_verify_batch(ctx._h, C.c_uint64(2), arr, bytes(32), status)
        rep = ctx.profile_report()
        ctx.profile_set(0)
        assert rc == 4, case
        assert list(status) == [77, 77] and all(ts.raw[:203] == state for ts in states), case
        assert rep == {}, case                                      # no launch
    assert lib.bpg_r1cs_verify_batch(ctx._h, C.c_uint64(0), None, None, None) == 0
    res.free()


def test_generator_capacity_is_per_item(small):
    c2 = bpg.Context(0)
    try:
        c2.gens_ensure(64)                                          # covers range56 (N = 64), not merkle4 (N = 8192)
        sub = [s for s in small if s[0] in ("range56", "merkle4")]
        st, _ = c2.verify_batch(_items(sub))
        assert st == [1 if s[0] == "merkle4" else 0 for s in sub]
    finally:
        c2.close()


def test_full_size_resident_items_mixed_with_flat_items(ctx):
    """cfg 3 (2^16, four dialects, bytes of proofs_big.json) as flat items and four 2^20 proofs of cfg 4 on the resident upload, in one batch"""
    a3 = GB.build("cfg3_mimc67", ctx)
    inst3, state3 = a3.prover.instance(), a3.transcript.state
    coms3 = b"".join(a3.commitments)
    ctx.gens_ensure(1 << 20)
    res3 = ctx.upload(inst3)
    recs3 = {r["flags"]: r for r in BIG if r["circuit"] == "cfg3_mimc67"}
    items = []
    for fl in range(4):
        proof, _ = res3.prove(state3, inst3.v_blinding, bytes.fromhex(recs3[fl]["seed"]), fl)
        assert hashlib.sha256(proof).hexdigest() == recs3[fl]["sha256"]
        items.append((inst3, state3, coms3, proof, SEED, fl))
    res3.free()
    a4 = GB.build("cfg4_merkle512", ctx)
    inst4, state4 = a4.prover.instance(), a4.transcript.state
    coms4 = b"".join(a4.commitments)
    res4 = ctx.upload(inst4)
    proofs4 = [res4.prove(state4, inst4.v_blinding, hashlib.sha256(b"batch %d" % k).digest(), 0)[0] for k in range(4)]
    assert len(set(proofs4)) == 4
    items += [(res4, state4, coms4, p, SEED, 0) for p in proofs4]
    ctx.profile_set(1)
    st, _ = ctx.verify_batch(items)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    assert st == [0] * 8 and rep["k_bucket_chunks"]["count"] == 1
    bad = bytearray(proofs4[2]); bad[len(bad) // 2] ^= 1
    tampered = list(items); tampered[6] = (res4, state4, coms4, bytes(bad), SEED, 0)
    assert ctx.verify_batch(tampered)[0] == [0] * 6 + [3, 0]
    badc = bytearray(coms3); badc[0] ^= 2
    flipped = list(items); flipped[1] = (inst3, state3, bytes(badc), items[1][3], SEED, 1)
    st, _ = ctx.verify_batch(flipped)
    assert st[1] == _verify_alone(ctx, inst3, state3, bytes(badc), items[1][3], SEED, 1)[0] != 0
    assert st[:1] + st[2:] == [0] * 7
    res4.free()


STEMS = ["bounds_check", "equality", "inequality", "less_than", "merkle_tree", "mimc_hash", "set_membership", "or", "or2", "or3", "or4", "or5", "example"]


def test_native_verifier_combine_prints_what_the_plain_batch_prints(tmp_path):
    prover_bin, verifier_bin = bpg_build.build_cli()
    env = dict(os.environ, BPG_CLI_SEED="cli-test", BPG_CLI_RNG_SEED="00" * 32)
    d = tmp_path / "stems"
    d.mkdir()
    for s in STEMS:
        for ext in ("gadgets", "inst", "wtns"):
            shutil.copy(ROOT / "tests" / "golden" / "resources" / ("%s.%s" % (s, ext)), d / ("%s.%s" % (s, ext)))
    (d / "batch.txt").write_text("\n".join(STEMS) + "\n")
    r = subprocess.run([str(prover_bin), "--batch", "batch.txt"], cwd=d, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(extra):
        return subprocess.run([str(verifier_bin), "--batch", "batch.txt"] + extra, cwd=d, env=env, capture_output=True, text=True, timeout=600)
    for tampered in (False, True):
        if tampered:
            bad = bytearray((d / "less_than.proof").read_bytes()); bad[40] ^= 1
            (d / "less_than.proof").write_bytes(bytes(bad))
        plain = run(["--workers", "1"])
        for extra in (["--workers", "1", "--combine"], ["--workers", "2", "--combine"]):
            got = run(extra)
            assert (got.returncode, got.stdout) == (plain.returncode, plain.stdout), (extra, got.stdout, got.stderr)
        if tampered:
            assert plain.returncode == 1 and "less_than: false" in plain.stdout and plain.stdout.count(": true") == len(STEMS) - 1
        else:
            assert plain.returncode == 0 and plain.stdout.strip().splitlines() == ["%s: true" % s for s in STEMS]
