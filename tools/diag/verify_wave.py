#!/usr/bin/env python3
"""Verifying K proofs of ONE resident circuit, two ways on one context, warm, generators built:
  new   ResidentCircuit.verify_batch (bpg_r1cs_verify_resident_batch): the replays on the host threads of the proving waves, a constant number of launches per
        wave, one MSM;
  old   what there was before, in the same process (this path is untouched):
          bounds    Context.verify_batch on the same items - per item a replay on one thread and seven stream operations, one MSM;
          inputs    per item ResidentCircuit.set_inputs + ResidentCircuit.verify (bpg_r1cs_verify_batch judges every item on the standing inputs, so K
                    different bounds were K calls each way).
Workloads: cfg 2 bounds checks (64-bit BoundsCheck, n = N = 128, m = 3) at K = 1, 64, 1024; LessThan against K different PUBLIC bounds (n = 379, N = 512, m = 3) at
K = 64, 1024.  The proofs are made once, outside the timed regions (prove_batch_commit / prove_batch_inputs), and every leg must accept every item.
Host clock around synchronised calls, the legs alternated (the order flips every repetition), median and min..max of --reps.  Beside each figure: the plan the new
call took (waves, chunks, launches per kernel, from the test hook on the same circuit and K) and, from one profiled call, the time of its kernels (HIP events) - the
rest of the wall time is the host's: replays, small scalars, copies, waits.
Writes one JSON object (profiles/verify_wave.json)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ms = lambda t0: (time.perf_counter() - t0) * 1e3
sc = lambda x: x.to_bytes(32, "little")


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bounds", default="1,64,1024")
    ap.add_argument("--inputs", default="64,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_wave.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    L = bpg.L
    ctx = bpg.Context(0)
    ctx.gens_ensure(512)
    rng = lambda k: hashlib.sha256(b"verify-wave prove %d" % k).digest()
    vseed = lambda k: hashlib.sha256(b"verify-wave verify %d" % k).digest()
    batch_seed = hashlib.sha256(b"verify-wave batch").digest()

    def before_commitments(label):
        t = bpg.Transcript(label); bpg.Prover(None, t)
        return t.state

    def verifier_state(label, coms):
        """the transcript as Verifier::new and every "V" append leave it"""
        t = bpg.Transcript(label); v = bpg.Verifier(t)
        for j in range(len(coms) // 32):
            v.commit(coms[32 * j:32 * j + 32])
        return t.state

    def hook_plan(tmpl, K, lgN, **kw):
        rec = [sc(3 + j) for j in range(7)] + [sc(2)] * lgN + [sc(pow(2, L - 2, L))] * lgN
        ev = tmpl.test_verify_wave_scalars([rec] * K, **kw)[3]
        return {k: ev[k] for k in ("waves", "items_per_wave", "chunks", "items_per_chunk", "target_blocks", "wave_bytes", "launches")}

    def measure(name, K, legs, want):
        for leg, fn in legs.items():                                       # warm: buffers grown, and every leg accepts every item
            assert fn() == want, "%s K = %d: %s does not accept every item" % (name, K, leg)
        T = {leg: [] for leg in legs}
        order = list(legs)
        for r in range(a.reps):
            for leg in (order if r % 2 == 0 else order[::-1]):
                t1 = time.perf_counter(); got = legs[leg](); T[leg].append(ms(t1))
                assert got == want, "%s K = %d repetition %d: %s" % (name, K, r, leg)
        out = {"items": K, "ms": {leg: spread(v) for leg, v in T.items()}}
        old = [leg for leg in legs if leg != "new"][0]
        out["ratio_old_over_new_median"] = round(out["ms"][old]["median"] / out["ms"]["new"]["median"], 2)
        out["new_median_below_old_range"] = out["ms"]["new"]["median"] < out["ms"][old]["min"]
        ctx.profile_set(2)
        t1 = time.perf_counter(); legs["new"](); wall = ms(t1)
        rep = ctx._report()
        ctx.profile_set(0)
        dev = sum(v.get("total_ms", 0.0) for v in rep.values())
        out["new_profiled_call"] = {"wall_ms": round(wall, 3), "kernels_ms": round(dev, 3), "host_and_waits_ms": round(wall - dev, 3),
                                    "vw_kernels_ms": round(sum(v.get("total_ms", 0.0) for k, v in rep.items() if k.startswith("k_vw_")), 3),
                                    "launches": {k: v.get("count") for k, v in rep.items() if k.startswith("k_vw_") or k in ("k_decompress", "k_bucket_chunks")}}
        return out

    out = {"source_hash": bench.source_hash(), "reps": a.reps, "clock": "host clock around synchronised calls, ms", "legs_alternated": True,
           "host_cpus_usable": len(os.sched_getaffinity(0)), "blocks_per_cu_constant": 4, "statuses": "every leg accepts every item, warm-up and every repetition",
           "bounds_check_64": [], "less_than_public_bound": []}

    # ---- cfg 2 bounds checks: one template, K witnesses, proofs and commitments from prove_batch_commit
    base = workloads.bounds_check_64(ctx, seed=0)
    tmpl = base.prover.template(ctx)
    lo, hi = bytes(8), b"\xff" * 8
    pre = before_commitments(b"BoundsCheck")

    def bounds_item(seed):
        cfg = "cfg2-%d" % seed
        t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(None, t); p.test_stub_commitments()
        blinds = [workloads.blinding(cfg, i) for i in range(3)]
        scalars, _, _ = bpg.commit(p, workloads.synth(cfg, 0, 8), blinds[:1])
        _, derived = bpg.BoundsCheck(lo, hi).setup(p, scalars, blinds[1:])
        return (b"".join(scalars) + b"".join(d[0] for d in derived), [], pre, b"".join(blinds), rng(seed), 0)

    Kmax = max(int(x) for x in a.bounds.split(","))
    proved = tmpl.prove_batch_commit([bounds_item(s) for s in range(1, Kmax + 1)])
    all_items = [(verifier_state(b"BoundsCheck", coms), coms, proof, vseed(k), 0) for k, (proof, _, coms) in enumerate(proved)]
    for K in [int(x) for x in a.bounds.split(",")]:
        items = all_items[:K]
        legs = {"new": lambda: tmpl.verify_batch(items, batch_seed=batch_seed)[0],
                "verify_batch": lambda: ctx.verify_batch([(tmpl,) + it for it in items], batch_seed=batch_seed)[0]}
        row = measure("bounds", K, legs, [0] * K)
        row["plan"] = hook_plan(tmpl, K, 7)
        out["bounds_check_64"].append(row)
        print(json.dumps(row), flush=True)
    tmpl.free()

    # ---- LessThan against K different public bounds: one template with the bound as a public input
    def statement(k):
        cfg = "verify-wave-lt-%d" % k
        bound = int.from_bytes(workloads.synth(cfg, 0, 15), "big") | (1 << 64) | k
        left = int.from_bytes(workloads.synth(cfg, 1, 15), "big") % bound
        delta = bound - left
        return bound, [sc(left), sc(delta), sc(pow(delta, L - 2, L))], [workloads.blinding(cfg, i) for i in range(3)]

    Kmax = max(int(x) for x in a.inputs.split(","))
    stmts = [statement(k) for k in range(Kmax)]
    assert len({b for b, _, _ in stmts}) == Kmax
    bound, values, blinds = stmts[0]
    tr = bpg.Transcript(b"LessThan"); p = bpg.Prover(ctx, tr)
    _, vs = p.commit_many(values, blinds)
    bpg.LessThan(vs[0], values[0], bpg.LinearCombination.of(p.input(sc(bound))), sc(bound)).prove(p, [], [(values[1], vs[1]), (values[2], vs[2])])
    tmpl = p.template(ctx)
    pre = before_commitments(b"LessThan")
    proved = tmpl.prove_batch_inputs([(b"".join(v), [], pre, b"".join(bl), rng(k), 0, None, [sc(b)]) for k, (b, v, bl) in enumerate(stmts)], commit=True)
    all_items = [(verifier_state(b"LessThan", r[2]), r[2], r[0], vseed(k), 0, None, sc(stmts[k][0])) for k, r in enumerate(proved)]
    for K in [int(x) for x in a.inputs.split(",")]:
        items = all_items[:K]

        def per_item():
            st = []
            for it in items:
                tmpl.set_inputs([it[6]])
                st.append(tmpl.verify(*it[:5]))
            return st
        legs = {"new": lambda: tmpl.verify_batch(items, batch_seed=batch_seed)[0], "set_inputs_and_verify_per_item": per_item}
        row = measure("inputs", K, legs, [0] * K)
        row["plan"] = hook_plan(tmpl, K, 9, inputs=[it[6] for it in items])
        out["less_than_public_bound"].append(row)
        print(json.dumps(row), flush=True)
    tmpl.free(); ctx.close()
    out["required"] = {"at K = 1024 the new call's median lies below the other leg's whole range, on both workloads":
                       all(r["new_median_below_old_range"] for w in ("bounds_check_64", "less_than_public_bound") for r in out[w] if r["items"] == 1024)}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
