#!/usr/bin/env python3
"""Which kernels a proof launches, how often, and with what roofline bookkeeping: the census that tests/test_launch_census_gpu.py compares with
tests/golden/launch_census.json.  Proof bytes cannot tell which fold kernel ran or how an MSM was planned - every choice gives the same bytes - so this
records, per case, every kernel's count, alg_bytes, device_bytes and field_mults from Context.profile_report() (never total_ms) and merged_last,
merged_skipped_last, shared_variants_last from Context.schedule().

Every case runs on a fresh Context(0) under profile_set(2), with fixed seeds and its knobs set in the environment while the context is created.  Every
case sets BPG_FOLD_ADAPT, and BPG_GENS_SHARE=0: the context then derives generator tables (and fold tables) of its own, so the counts of the
table-building kernels do not depend on what other contexts of the process hold at the time.

  a  MiMC preimage of 100 bytes (n = 3,888, N = 4,096), bucket-method path (BPG_TT_LG=0), a proof alone: one prove, one verify
  b  500 bytes (N = 16,384), the shared-device variants (BPG_FOLD_ADAPT=2): one prove, one verify
  c  20 bytes (N = 1,024), no split kernels, width-5 NAF fold tables on scalars cut in two: one prove, one verify
  d  300 identical multipliers beside a 200-bit range proof (N = 512), equal scalars merged (BPG_MERGE=1): two proofs on one upload
  e  the circuit of (a) with default knobs (the table-driven path: no MSM in the argument): one prove, one verify

Uses the public Python API only.  `launch_census.py --out FILE` writes the census of all cases as JSON (the golden file is a recording of the commit
BEFORE the MSM and fold planners moved into host/msm_plan.hpp and host/fold_plan.hpp)."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEED = bytes(range(32))
SUMS = ("alg_bytes", "device_bytes", "field_mults")
SCHEDULE_KEYS = ("merged_last", "merged_skipped_last", "shared_variants_last")


def _mimc(nbytes, seed):
    def build(bpg, workloads, ctx):
        a = workloads.mimc_preimage(ctx, nbytes=nbytes, seed=seed, label=b"MiMCHash")
        return a.prover, a.transcript, a.commitments, a.gens_capacity
    return build


def _skewed(bpg, workloads, ctx):
    """tests/test_gpu_parity.py test_skewed_witness_distributions: range-proof bits and 300 multipliers with identical assignments"""
    sc = lambda x: (x % bpg.L).to_bytes(32, "little")
    t = bpg.Transcript(b"skew")
    p = bpg.Prover(ctx, t)
    x = (2**200 - 12345).to_bytes(32, "little")
    cs, vs = p.commit_many([x], [sc(0x5eed)])
    bpg.range_proof(p, vs[0], 200, x)
    for _ in range(300):
        l, r, o = p.allocate_multiplier((sc(7), sc(9)))
        p.constrain(bpg.LinearCombination.of(o) - sc(63))
    return p, t, cs, 512


# name -> (environment, circuit, proofs, verify)
CASES = {
    "a": ({"BPG_TT_LG": "0", "BPG_FOLD_ADAPT": "0"}, _mimc(100, 21), 1, True),
    "b": ({"BPG_TT_LG": "0", "BPG_FOLD_ADAPT": "2"}, _mimc(500, 22), 1, True),
    "c": ({"BPG_TT_LG": "0", "BPG_FOLD_SPLIT": "0", "BPG_FOLD_WNAF": "5", "BPG_FOLD_PARTS": "2", "BPG_FOLD_ADAPT": "0"}, _mimc(20, 3), 1, True),
    "d": ({"BPG_TT_LG": "0", "BPG_MERGE": "1", "BPG_FOLD_ADAPT": "0"}, _skewed, 2, False),
    "e": ({"BPG_FOLD_ADAPT": "1"}, _mimc(100, 21), 1, True),
}


@contextlib.contextmanager
def _environment(env):
    """the case's knobs and nothing else of BPG_*: the context reads them once, when it is created"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("BPG_") and k not in ("BPG_LIB_PATH", "BPG_REBUILD")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env, BPG_GENS_SHARE="0")
    try:
        yield
    finally:
        for k in list(env) + ["BPG_GENS_SHARE"]:
            del os.environ[k]
        os.environ.update(saved)


def run_case(name):
    """{"kernels": {kernel: {count, alg_bytes, device_bytes, field_mults}}, "schedule": {...}} of one case"""
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    env, circuit, proofs, verify = CASES[name]
    with _environment(env):
        ctx = bpg.Context(0)
    try:
        ctx.profile_set(2)
        prover, transcript, commitments, cap = circuit(bpg, workloads, ctx)
        inst = prover.instance()
        ctx.gens_ensure(cap)
        res = ctx.upload(inst)
        for _ in range(proofs):
            proof, _state = res.prove(transcript.state, inst.v_blinding, SEED, 0)
        if verify:
            assert res.verify(transcript.state, b"".join(commitments), proof) == 0, "case %s: the proof was rejected" % name
        report, schedule = ctx.profile_report(), ctx.schedule()
        res.free()
    finally:
        ctx.close()
    return {"kernels": {k: {"count": v["count"], **{s: v[s] for s in SUMS}} for k, v in sorted(report.items())},
            "schedule": {k: schedule[k] for k in SCHEDULE_KEYS}}


def census():
    return {name: run_case(name) for name in CASES}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_census.json"))
    a = ap.parse_args()
    got = census()
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in got.items():
        folds = {k: v["count"] for k, v in c["kernels"].items() if k.startswith("k_fold_points")}
        print(name, "kernels", len(c["kernels"]), "launches", sum(v["count"] for v in c["kernels"].values()), "folds", folds, c["schedule"])
