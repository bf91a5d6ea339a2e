"""Template batches that make their own Pedersen commitments on the GPU (bpg_r1cs_prove_template_batch_commit, k_bt_commit_v): from (values, blindings,
transcript as Prover::new leaves it) to (commitments, proofs, transcripts) in one call.

The new path is never compared with itself.  Commitments are compared with the CPU oracle's pedersen_commit (tests/oracle_lib.py) and with
bpg_pedersen_commit; proofs and out-states with the EXISTING ResidentCircuit.prove_batch fed the post-commit states a prover made the existing way
(Prover.commit per value); the oracle's verifier judges proofs against the returned commitments.

Circuit: the hinted 64-bit BoundsCheck template (n = N = 128, m = 3) unless said otherwise.

Run as a script (`python tests/test_template_commit_gpu.py child [expanded]`) the file proves the 64-item batch through the new call under the environment
it was started with and prints commitments, proofs, states and launch counts as JSON, after the launch counts of the EXISTING prove_batch on the same
items under the same environment: the wave cut and the fallback are read at context creation."""
import ctypes as C
import json
import os
import pathlib
import subprocess
import sys

if __name__ == "__main__":
    _root = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "tests"), str(_root / "tests" / "golden")]

import pytest
import bulletproofs_gadgets_amd as bpg
from test_template_hints_gpu import bounds_case, bounds_with, Case, rng

pytestmark = pytest.mark.gpu
L = bpg.L
ROOT = pathlib.Path(__file__).resolve().parent.parent
SEEDS = list(range(100, 230))            # the first 64 are the witnesses of tests/test_template_hints_gpu.py
sc = lambda x: x.to_bytes(32, "little")


def state_before(label):
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(label)
    bpg.Prover(None, t)
    return t.state


def commit_item(c, pre, flags=0, params=()):
    return (c.inst.v, list(params), pre, c.inst.v_blinding, rng(c.tag), flags)


def launches(ctx, call, items):
    ctx.profile_set(2)
    res = call(items)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    return res, {k: rep.get(k, {"count": 0})["count"] for k in ("k_bt_commit_v", "k_pedersen", "k_witness_eval_batch", "k_witness_eval")}


def _child(expanded):
    ctx = bpg.Context(0)
    ctx.gens_ensure(128)
    cases = [bounds_case(ctx, s) for s in SEEDS[:64]]
    tmpl = cases[0].a.prover.template(ctx)
    pre = state_before(b"BoundsCheck")
    flags = [4 if (expanded and k == 20) else 0 for k in range(64)]
    _, old = launches(ctx, tmpl.prove_batch, [(c.inst.v, [], c.state, c.inst.v_blinding, rng(c.tag), f) for c, f in zip(cases, flags)])
    res, n = launches(ctx, tmpl.prove_batch_commit, [commit_item(c, pre, flags=f) for c, f in zip(cases, flags)])
    print(json.dumps({"proofs": [p.hex() for p, _, _ in res], "states": [s.hex() for _, s, _ in res], "coms": [c.hex() for _, _, c in res], "launches": n,
                      "existing": old}))
    tmpl.free(); ctx.close()


if __name__ == "__main__":
    _child(len(sys.argv) > 2 and sys.argv[2] == "expanded")
    sys.exit(0)

import oracle_lib as O
from test_template_gpu import constant_term, last_row, to_oracle
from test_template_commit_host import commit_items


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(1 << 14)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pre():
    return state_before(b"BoundsCheck")


@pytest.fixture(scope="module")
def bounds(ctx):
    """130 witnesses assembled the existing way (three Prover.commit calls each): their post-commit states feed the existing prove_batch"""
    return [bounds_case(ctx, s) for s in SEEDS]


@pytest.fixture(scope="module")
def oracle_coms(bounds):
    """the oracle's commitments of every witness, computed once"""
    out = []
    for c in bounds:
        out.append(b"".join(O.pedersen_commit(c.inst.v[32 * j:32 * j + 32], c.inst.v_blinding[32 * j:32 * j + 32]) for j in range(3)))
    return out


@pytest.fixture(scope="module")
def tmpl(ctx, bounds):
    t = bounds[0].a.prover.template(ctx)
    yield t
    t.free()


@pytest.fixture(scope="module")
def want130(tmpl, bounds):
    """the existing call on the host-made post-commit states: (proof, state after) per witness - an item's bytes do not depend on its batch
    (tests/test_template_batch_gpu.py), so one batch of 130 serves every K"""
    return tmpl.prove_batch([c.item() for c in bounds])


@pytest.mark.parametrize("K", [1, 3, 65, 130])
def test_bytes(ctx, tmpl, bounds, oracle_coms, want130, pre, K):
    assert bounds[0].inst.n == 128 and bounds[0].inst.m == 3 and bounds[0].state != pre
    got = tmpl.prove_batch_commit([commit_item(c, pre) for c in bounds[:K]])
    assert len(got) == K
    for k, (proof, state, coms) in enumerate(got):
        assert coms == oracle_coms[k], "item %d of %d: the commitments differ from the oracle's" % (k, K)
        assert coms == bounds[k].coms
        assert (proof, state) == want130[k], "item %d of %d: proof or out-state differ from the existing prove_batch" % (k, K)
    ogens = O.Gens(128)
    for k in sorted({0, K // 2, K - 1}):
        c = bounds[k]
        assert O.verify(ogens, c.state, to_oracle(c.inst), got[k][2], got[k][0]) == 0, "item %d: the oracle rejects the proof" % k


NIB8 = int("0" + "8" * 63, 16)
NIB9V = int("1" + "9" * 63, 16)          # every nibble 9 below the top one: a value stays below 2^255
NIB9 = int("9" * 64, 16)
TOP = (8 * 16 ** 63) % L
EDGE_PAIRS = [(0, 0), (1, 0), (0, 1), (L - 1, L - 1), (L, L), ((1 << 255) - 1, (1 << 255) | 12345), (NIB8, NIB8), (NIB9V, NIB9), (TOP, TOP),
              (NIB8, 1), (1, NIB9), (L - 1, 0)]


def test_edge_scalars(ctx, tmpl, pre):
    """values and blindings at the corners of the digit recoding and of the reduction, three pairs per item; the witnesses they imply are out of range
    and only the commitments are compared: with the oracle (given the scalars reduced mod l - B and B_blinding have order l) and with
    bpg_pedersen_commit (given the raw bytes)"""
    assert all(v < (1 << 255) for v, _ in EDGE_PAIRS) and len(EDGE_PAIRS) % 3 == 0
    items = []
    for k in range(0, len(EDGE_PAIRS), 3):
        v = b"".join(sc(a) for a, _ in EDGE_PAIRS[k:k + 3]); r = b"".join(sc(b) for _, b in EDGE_PAIRS[k:k + 3])
        items.append((v, [], pre, r, rng("edge %d" % k), 0))
    got = tmpl.prove_batch_commit(items)
    flat = b"".join(c for _, _, c in got)
    ours = ctx.pedersen_commit([sc(a) for a, _ in EDGE_PAIRS], [sc(b) for _, b in EDGE_PAIRS])
    for j, (a, b) in enumerate(EDGE_PAIRS):
        com = flat[32 * j:32 * j + 32]
        assert com == O.pedersen_commit(sc(a % L), sc(b % L)), "pair %d (%x, %x): the oracle's commitment" % (j, a, b)
        assert com == ours[j], "pair %d (%x, %x): bpg_pedersen_commit" % (j, a, b)
    assert flat[:32] == bytes(32) and flat[32 * 4:32 * 5] == bytes(32)       # 0 B + 0 B~ and l B + l B~: the identity encodes as zero bytes
    assert len(set(flat[32 * j:32 * j + 32] for j in range(len(EDGE_PAIRS)))) == len(EDGE_PAIRS) - 1


def test_merkle_template_with_a_parameter_row_and_mixed_dialects(ctx):
    """m = 8 and one parameter row: the 8-leaf Merkle template of tests/test_template_batch_gpu.py, four items under the four dialect flags"""
    from test_template_batch_gpu import Case as Tree, make_template, rng as tree_rng
    trees = [Tree(ctx, s) for s in (2, 3, 4, 5)]
    t = make_template(ctx, trees[0])
    mpre = state_before(b"MerkleTree")
    want = t.prove_batch([c.item(flags=k) for k, c in enumerate(trees)])
    got = t.prove_batch_commit([(c.inst.v, [c.param], mpre, c.inst.v_blinding, tree_rng(c.seed), k) for k, c in enumerate(trees)])
    ogens = O.Gens(1 << 14)
    for k, (c, (proof, state, coms)) in enumerate(zip(trees, got)):
        assert len(coms) == 8 * 32
        assert coms == b"".join(O.pedersen_commit(c.inst.v[32 * j:32 * j + 32], c.inst.v_blinding[32 * j:32 * j + 32]) for j in range(8)), "tree %d" % k
        assert coms == b"".join(c.a.commitments)
        assert (proof, state) == want[k], "tree %d under flags %d" % (k, k)
    assert O.verify(ogens, trees[0].state, to_oracle(trees[0].inst), got[0][2], got[0][0]) == 0
    t.free()


def run_child(env, *args):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_template_commit_gpu.py"), "child"] + list(args), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", ["several-waves", "fallback", "expanded-among-lockstep"])
def test_waves_and_fallback(ctx, tmpl, bounds, oracle_coms, want130, setting):
    """The child counts the launches of the EXISTING prove_batch on the same 64 items under the same environment first: k_witness_eval_batch runs once
    per wave there (the template has one schedule level), and the wave cut does not depend on who makes the commitments.  The new call must launch
    k_bt_commit_v exactly that often, k_witness_eval_batch and k_witness_eval exactly as the existing call does, and k_pedersen as often plus the
    ONE launch that makes the commitments of all the items off the lockstep path.  BPG_BATCH_WAVE_MB=1: several waves.  BPG_TT_ORIG_LG=0: no lockstep
    path - k_bt_commit_v never runs.  One item with BPG_FLAG_EXPANDED_BLINDING: it alone leaves the lockstep path, the other 63 share one wave."""
    env = {"several-waves": {"BPG_BATCH_WAVE_MB": "1"}, "fallback": {"BPG_TT_ORIG_LG": "0"}, "expanded-among-lockstep": {}}[setting]
    out = run_child(env, *(["expanded"] if setting == "expanded-among-lockstep" else []))
    n, old = out["launches"], out["existing"]
    print(setting, n, old)
    waves, singles = {"several-waves": (None, 0), "fallback": (0, 64), "expanded-among-lockstep": (1, 1)}[setting]
    assert old["k_bt_commit_v"] == 0 and old["k_witness_eval"] == singles and (old["k_witness_eval_batch"] > 1 if waves is None else old["k_witness_eval_batch"] == waves), old
    assert n["k_bt_commit_v"] == old["k_witness_eval_batch"], (n, old)            # one launch per wave, exactly
    assert n["k_witness_eval_batch"] == old["k_witness_eval_batch"] and n["k_witness_eval"] == old["k_witness_eval"], (n, old)
    assert n["k_pedersen"] == old["k_pedersen"] + (1 if singles else 0), (n, old)
    want = list(want130[:64])
    if setting == "expanded-among-lockstep":
        c = bounds[20]
        want[20] = tmpl.prove_batch([(c.inst.v, [], c.state, c.inst.v_blinding, rng(c.tag), 4)])[0]
    for k in range(64):
        assert bytes.fromhex(out["coms"][k]) == oracle_coms[k], "item %d: commitments" % k
        assert (bytes.fromhex(out["proofs"][k]), bytes.fromhex(out["states"][k])) == want[k], "item %d: proof or out-state" % k


def test_launches_do_not_grow_with_k(ctx, tmpl, bounds, want130, pre):
    for K in (8, 64):
        _, old = launches(ctx, tmpl.prove_batch, [c.item() for c in bounds[:K]])
        got, new = launches(ctx, tmpl.prove_batch_commit, [commit_item(c, pre) for c in bounds[:K]])
        assert new["k_bt_commit_v"] == 1 and old["k_bt_commit_v"] == 0, (K, new, old)
        assert new["k_pedersen"] == old["k_pedersen"], (K, new, old)         # the commitments of t_1, t_3 .. t_6 only, as before
        assert new["k_witness_eval_batch"] == old["k_witness_eval_batch"] == 1
        assert [(p, s) for p, s, _ in got] == want130[:K]


def test_an_item_fails_alone(ctx, tmpl, bounds, oracle_coms, want130, pre):
    items = [commit_item(c, pre) for c in bounds[:6]]
    arr, keep, coms = commit_items(tmpl, items)
    keep[1][2].value -= 1                                                    # a proof buffer one byte short
    arr[2].commitments_out = None                                            # NULL commitments_out
    arr[4].v_blinding = None                                                 # NULL blinding
    status = (C.c_int32 * 6)(*[77] * 6)
    rc = bpg.lib().bpg_r1cs_prove_template_batch_commit(ctx._h, tmpl._h, C.c_uint64(6), arr, status)
    assert rc == 4 and list(status) == [0, 4, 4, 0, 4, 0], list(status)
    assert b"item 1" in bpg.lib().bpg_last_error()
    for k in range(6):
        ts, out, ln = keep[k][:3]
        if k in (1, 2, 4):
            assert ts.raw[:203] == pre, "item %d: a failed item's transcript is left as given" % k
            assert coms[k].raw == b"\xa5" * 96, "item %d: no commitment is written for a failed item" % k
        else:
            assert coms[k].raw == oracle_coms[k], "item %d: commitments" % k
            assert (out.raw[:ln.value], ts.raw[:203]) == want130[k], "item %d: proof or out-state" % k
    items[3] = items[3][:3] + (None,) + items[3][4:]                         # the binding's conventions for a failed item
    res, st = tmpl.prove_batch_commit(items, return_status=True)
    assert st == [0, 0, 0, 4, 0, 0] and res[3] == (None, pre, None)
    assert res[0] == want130[0] + (oracle_coms[0],)


def test_template_state_afterwards(ctx, tmpl, bounds, want130, pre):
    c = bounds[2]
    assert c.assign_and_prove(tmpl) == c.host_proof()                        # a witness is resident ...
    tmpl.prove_batch_commit([commit_item(bounds[3], pre), commit_item(bounds[4], pre)])
    with pytest.raises(bpg.BpgError) as e:                                   # ... and gone after a batch: MISSING_ASSIGNMENT until the next assign
        tmpl.prove(c.state, c.inst.v_blinding, rng(c.tag))
    assert e.value.status == 5
    assert c.assign_and_prove(tmpl) == c.host_proof()
    assert tmpl.prove_batch_commit([]) == []                                 # count == 0 is BPG_OK and touches nothing ...
    assert bpg.lib().bpg_r1cs_prove_template_batch_commit(ctx._h, tmpl._h, C.c_uint64(0), None, None) == 0     # ... without items or status_out either
    assert tmpl.prove(c.state, c.inst.v_blinding, rng(c.tag)) == c.host_proof()
    plain = ctx.upload(c.inst)
    with pytest.raises(bpg.BpgError) as e:                                   # not a template: the whole call is refused
        plain.prove_batch_commit([commit_item(c, pre)])
    assert e.value.status == 4
    plain.free()
