"""Range-proof templates on the GPU (bit hints, bpg_r1cs_upload_template_hinted): a hinted template that is assigned fresh committed values - one at a
time (k_witness_eval) or K in lockstep (k_witness_eval_batch) - proves exactly what the EXISTING path proves for the same witness: host assembly,
bpg_r1cs_upload, bpg_r1cs_prove_resident.  Proof bytes and transcript states are compared with that path everywhere, never with the template itself; the
GPU verifier and the CPU oracle's verifier judge the proofs.

Circuits: BoundsCheck over [0, 2^64) (n = N = 128, one schedule level), LessThan over two committed values (n = 379, N = 512, one level), and a two-leaf
Merkle node followed by a 64-bit range proof over its hash (n = 2008, N = 2048, three levels; the statement is false - a hash is no 64-bit number - and
only its bytes are compared).

Run as a script (`python tests/test_template_hints_gpu.py child`) the file proves the 64-item BoundsCheck batch under the environment it was started with
and prints proofs and launch counts as JSON: how the wave cut and the one-at-a-time fallback, both read at context creation, are exercised."""
import hashlib
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
from bulletproofs_gadgets_amd import workloads

pytestmark = pytest.mark.gpu
L = bpg.L
ROOT = pathlib.Path(__file__).resolve().parent.parent
SEEDS64 = list(range(100, 164))
sc = lambda x: x.to_bytes(32, "little")


def rng(tag):
    return hashlib.sha256(("template hints %s" % tag).encode()).digest()


def bounds_with(ctx, values, tag):
    """BoundsCheck over [0, 2^64) for ANY committed (witness, a, b): what an out-of-range witness needs"""
    t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
    coms, vs = p.commit_many(values, [workloads.blinding(tag, i) for i in range(3)])
    bpg.BoundsCheck(bytes(8), b"\xff" * 8).prove(p, vs[:1], [(values[1], vs[1]), (values[2], vs[2])])
    return workloads.Assembled(p, t, coms, 128, None)


def mixed(ctx, seed):
    t = bpg.Transcript(b"mixed"); p = bpg.Prover(ctx, t)
    leaves = [sc(int.from_bytes(workloads.synth("mixed-%d" % seed, i), "little") % L) for i in range(2)]
    coms, vs = p.commit_many(leaves, [workloads.blinding("mixed-%d" % seed, i) for i in range(2)])
    bpg.MerkleTree256(bytes(32), [], bpg.vars_to_lc(vs), "(W W)").prove(p, [], [])
    n0 = p.get_num_multiplications()
    bpg.range_proof(p, bpg.Variable(2 << 29 | (n0 - 1)), 64, p.instance().aO[-32:])
    return workloads.Assembled(p, t, coms, 2048, None)


class Case:
    """one witness: its host assembly, and the existing path's (proof, transcript state after), made on demand"""
    def __init__(self, ctx, a, tag):
        self.ctx, self.a, self.tag = ctx, a, tag
        self.inst = a.prover.instance()
        self.state = a.transcript.state
        self.coms = b"".join(a.commitments)
        self._want = None

    def item(self, flags=0):
        return (self.inst.v, [], self.state, self.inst.v_blinding, rng(self.tag), flags)

    def host_proof(self):
        if self._want is None:
            res = self.ctx.upload(self.inst)
            self._want = res.prove(self.state, self.inst.v_blinding, rng(self.tag))
            res.free()
        return self._want

    def assign_and_prove(self, tmpl):
        tmpl.assign(self.inst.v)
        return tmpl.prove(self.state, self.inst.v_blinding, rng(self.tag))


def bounds_case(ctx, seed):
    return Case(ctx, workloads.bounds_check_64(ctx, seed=seed), "bounds %d" % seed)


def witness_launches(ctx, tmpl, items):
    ctx.profile_set(2)
    res = tmpl.prove_batch(items)
    rep = ctx.profile_report()
    ctx.profile_set(0)
    return res, rep.get("k_witness_eval_batch", {"count": 0})["count"], rep.get("k_witness_eval", {"count": 0})["count"]


def _child():
    ctx = bpg.Context(0)
    ctx.gens_ensure(128)
    cases = [bounds_case(ctx, s) for s in SEEDS64]
    tmpl = cases[0].a.prover.template(ctx)
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [c.item() for c in cases])
    print(json.dumps({"proofs": [p.hex() for p, _ in res], "states": [s.hex() for _, s in res], "nbatch": nbatch, "nsingle": nsingle}))
    tmpl.free(); ctx.close()


if __name__ == "__main__":
    _child()
    sys.exit(0)

import oracle_lib as O
from test_template_gpu import to_oracle


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(2048)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bounds64(ctx):
    return [bounds_case(ctx, s) for s in SEEDS64]


def oracle_accepts(ogens, c, proof):
    return O.verify(ogens, c.state, to_oracle(c.inst), c.coms, proof) == 0


def test_bounds_check_single_path(ctx):
    base = bounds_case(ctx, 1)
    assert base.inst.n == 128
    tmpl = base.a.prover.template(ctx)
    assert tmpl.n_params == 0
    assert tmpl.prove(base.state, base.inst.v_blinding, rng(base.tag)) == base.host_proof()        # the uploaded witness: no assign needed
    ogens = O.Gens(128)
    for seed in (2, 3, 4, 5, 6):
        c = bounds_case(ctx, seed)
        assert c.inst.v != base.inst.v
        got = c.assign_and_prove(tmpl)
        assert got == c.host_proof(), "seed %d: the assigned template and the host assembly give different proofs" % seed
        assert tmpl.verify(c.state, c.coms, got[0]) == 0, "seed %d: verify_resident on the template" % seed
        assert oracle_accepts(ogens, c, got[0]), "seed %d: the oracle rejects the proof" % seed
    tmpl.free()


def test_bounds_check_batch_of_64(ctx, bounds64):
    tmpl = bounds64[0].a.prover.template(ctx)
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [c.item() for c in bounds64])
    assert (nbatch, nsingle) == (1, 0), "one level, one wave: one shared launch"
    ogens = O.Gens(128)
    for c, got in zip(bounds64, res):
        assert got == c.host_proof(), "%s: the template batch and the host assembly differ" % c.tag
    for c, got in list(zip(bounds64, res))[::16]:
        assert oracle_accepts(ogens, c, got[0]) and ctx.verify_flat(c.inst, c.state, c.coms, got[0]) == 0
    with pytest.raises(bpg.BpgError) as e:                                   # no witness afterwards, as documented for any template batch
        tmpl.prove(bounds64[0].state, bounds64[0].inst.v_blinding, rng(bounds64[0].tag))
    assert e.value.status == 5
    for c in bounds64[:3]:                                                   # ... and the single path gives the same bytes
        assert c.assign_and_prove(tmpl) == c.host_proof()
    tmpl.free()


def run_child(env):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_template_hints_gpu.py"), "child"], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", ["several-waves", "one-at-a-time"])
def test_batch_of_64_in_waves_and_through_the_fallback(bounds64, setting):
    """BPG_BATCH_WAVE_MB=1: the engine counts 28 N x 32 B = 114,688 B of device state per item plus rows, terms and coefficients of the instance (259 rows
    at 48 B, under 700 terms at 24 B, under 100 coefficients at 64 B: under 37 KB) - between 112 and 150 KB, so a wave of 1 MB holds 7 to 9 items and the
    64 items run in 8 to 10 waves, one launch of k_witness_eval_batch each (one level).  BPG_TT_ORIG_LG=0: no lockstep path, every item is assign +
    prove_resident inside the call: 64 launches of k_witness_eval."""
    out = run_child({"BPG_BATCH_WAVE_MB": "1"} if setting == "several-waves" else {"BPG_TT_ORIG_LG": "0"})
    print(setting, "k_witness_eval_batch:", out["nbatch"], "k_witness_eval:", out["nsingle"])
    if setting == "several-waves":
        assert out["nsingle"] == 0 and 8 <= out["nbatch"] <= 10, out["nbatch"]
    else:
        assert (out["nbatch"], out["nsingle"]) == (0, 64)
    for k, c in enumerate(bounds64):
        want = c.host_proof()
        assert (bytes.fromhex(out["proofs"][k]), bytes.fromhex(out["states"][k])) == want, c.tag


@pytest.mark.parametrize("kind", ["less_than", "mixed"])
def test_less_than_and_mixed_circuits(ctx, kind):
    make = (lambda s: workloads.less_than_126(ctx, seed=s)) if kind == "less_than" else (lambda s: mixed(ctx, s))
    cases = [Case(ctx, make(s), "%s %d" % (kind, s)) for s in range(1, 8)]
    assert cases[0].inst.n == (379 if kind == "less_than" else 2008)
    tmpl = cases[0].a.prover.template(ctx)
    for c in cases[1:4]:
        assert c.assign_and_prove(tmpl) == c.host_proof(), "%s: single path" % c.tag
    res, nbatch, nsingle = witness_launches(ctx, tmpl, [c.item() for c in cases])
    assert (nbatch, nsingle) == ((1, 0) if kind == "less_than" else (3, 0))
    for c, got in zip(cases, res):
        assert got == c.host_proof(), "%s: batch" % c.tag
    if kind == "less_than":
        ogens = O.Gens(512)
        for c, got in zip(cases, res):
            assert oracle_accepts(ogens, c, got[0]) and ctx.verify_flat(c.inst, c.state, c.coms, got[0]) == 0, c.tag
    tmpl.free()


def test_out_of_range_witness(ctx, bounds64):
    """a = 2^64 + 5 and b = 2^64 - 1 - a: the linear constraint a + b = max - min holds, the range proof of a does not.  Bits above bit 63 are ignored by
    the host and by the device alike: same witness, same bytes, and a proof the verifier rejects - alone in its batch."""
    a = (1 << 64) + 5
    bad = Case(ctx, bounds_with(ctx, [sc(7), sc(a), sc(((1 << 64) - 1 - a) % L)], "oob"), "oob")
    tmpl = bounds64[0].a.prover.template(ctx)
    got = bad.assign_and_prove(tmpl)
    assert got == bad.host_proof()
    assert tmpl.verify(bad.state, bad.coms, got[0]) == 3                      # BPG_ERR_VERIFICATION
    assert ctx.verify_flat(bad.inst, bad.state, bad.coms, got[0]) == 3
    batch = bounds64[:5] + [bad] + bounds64[5:10]
    res = tmpl.prove_batch([c.item() for c in batch])
    for c, r in zip(batch, res):
        assert r == c.host_proof(), c.tag
        assert ctx.verify_flat(c.inst, c.state, c.coms, r[0]) == (3 if c is bad else 0), c.tag
    assert O.verify(O.Gens(128), bad.state, to_oracle(bad.inst), bad.coms, res[5][0]) != 0
    tmpl.free()
