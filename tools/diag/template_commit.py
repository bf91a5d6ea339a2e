#!/usr/bin/env python3
"""K 64-bit BoundsCheck witnesses of one hinted template, from (values, blindings) to proofs, three ways on one context:
  (a) what there was before: per item a Transcript and a Prover, three Prover.commit calls (a k_pedersen launch and a round trip each), then
      ResidentCircuit.prove_batch on the post-commit states;
  (b) what a careful caller could already do: ONE Context.pedersen_commit of all 3 K values, per item the three "V" appends through the binding
      (Prover.commit_precomputed on a device-less prover), then prove_batch;
  (c) ResidentCircuit.prove_batch_commit: the commitments of a wave in one launch of k_bt_commit_v inside the call.
Host clock around calls that end synchronised, the three ways rotated in every repetition, median of --reps after one warm-up repetition in which the
proofs, states and commitments of the three ways are compared byte for byte.  The values and blindings are derived once, outside the timed regions, for
(b) and (c); (a) derives them inside its loop, as its callers did (Gadget.setup).
Then, in passes of their own with the engine's event profile on: the device time of k_bt_commit_v at K m = 3 K commitments for 1, 2 and 4
commitments per wave of the kernel (BPG_COMMIT_CPW, read at context creation, so each setting gets a context of its own), beside one k_pedersen launch of the same count.  Prints one JSON object (kept as profiles/template_commit.json)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", default="serving")
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads

    def context():
        c = bpg.Context(0, profile=a.profile) if a.profile else bpg.Context(0)
        c.gens_ensure(128)
        return c
    ctx = context()
    rng = lambda k: hashlib.sha256(b"template commit %d" % k).digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    lo, hi = bytes(8), b"\xff" * 8

    def commitments(seed):
        """the commitments and the transcript of workloads.bounds_check_64 without its assembly -> (values, blindings, transcript state, commitments)"""
        cfg = "cfg2-%d" % seed
        t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
        blinds = [workloads.blinding(cfg, i) for i in range(3)]
        scalars, wcoms, _ = bpg.commit(p, workloads.synth(cfg, 0, 8), blinds[:1])
        dcoms, derived = bpg.BoundsCheck(lo, hi).setup(p, scalars, blinds[1:])
        return b"".join(scalars) + b"".join(d[0] for d in derived), b"".join(blinds), t.state, b"".join(wcoms + dcoms)

    t = bpg.Transcript(b"BoundsCheck"); bpg.Prover(None, t)
    pre = t.state
    base = workloads.bounds_check_64(ctx, seed=0)
    out = {"circuit": "bounds_check_64", "n": base.prover.get_num_multiplications(), "m": 3, "reps": a.reps, "profile": a.profile,
           "conditions": {"device": "device 0 of the node (one GPU, nothing else of this process on it, clocks as the driver leaves them)",
                          "host_cpus_usable": len(os.sched_getaffinity(0)),
                          "method": "host perf_counter around calls that end synchronised; the three ways rotated per repetition, median of reps after one "
                          "checked warm-up; kernels: HIP-event profile, one launch per sample, median of reps"},
           "sizes": {}}
    for K in [int(x) for x in a.sizes.split(",")]:
        seeds = list(range(1, K + 1))
        known = [commitments(s) for s in seeds]                 # values and blindings of (b) and (c), and the commitments all three must reach
        vals, blinds = [k[0] for k in known], [k[1] for k in known]
        tmpl = base.prover.template(ctx)
        T = {"a_commit_ms": [], "a_prove_batch_ms": [], "b_commit_ms": [], "b_append_ms": [], "b_prove_batch_ms": [], "c_prove_batch_commit_ms": []}
        for rep in range(a.reps + 1):
            for way in [(0, 1, 2), (1, 2, 0), (2, 0, 1)][rep % 3]:
                if way == 0:
                    t0 = time.perf_counter(); com = [commitments(s) for s in seeds]; ta_com = ms(t0)
                    items = [(v, [], state, vb, rng(s), 0) for (v, vb, state, _), s in zip(com, seeds)]
                    t0 = time.perf_counter(); got_a = tmpl.prove_batch(items); ta_prove = ms(t0)
                elif way == 1:
                    t0 = time.perf_counter()
                    flat = ctx.pedersen_commit([v[32 * j:32 * j + 32] for v in vals for j in range(3)], [b[32 * j:32 * j + 32] for b in blinds for j in range(3)])
                    tb_com = ms(t0)
                    t0 = time.perf_counter()
                    states = []
                    for k in range(K):
                        tr = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(None, tr)
                        for j in range(3):
                            p.commit_precomputed(vals[k][32 * j:32 * j + 32], blinds[k][32 * j:32 * j + 32], flat[3 * k + j])
                        states.append(tr.state)
                    tb_app = ms(t0)
                    items = [(vals[k], [], states[k], blinds[k], rng(s), 0) for k, s in enumerate(seeds)]
                    t0 = time.perf_counter(); got_b = tmpl.prove_batch(items); tb_prove = ms(t0)
                else:
                    items = [(vals[k], [], pre, blinds[k], rng(s), 0) for k, s in enumerate(seeds)]
                    t0 = time.perf_counter(); got_c = tmpl.prove_batch_commit(items); tc = ms(t0)
            if rep == 0:
                assert got_b == got_a, "one pedersen_commit + appends and the per-item commits give different proofs"
                assert [(p, s) for p, s, _ in got_c] == got_a, "prove_batch_commit and the per-item commits give different proofs"
                assert [c for _, _, c in got_c] == [k[3] for k in known] == [b"".join(flat[3 * k:3 * k + 3]) for k in range(K)], "commitments differ"
                continue
            for key, v in (("a_commit_ms", ta_com), ("a_prove_batch_ms", ta_prove), ("b_commit_ms", tb_com), ("b_append_ms", tb_app),
                           ("b_prove_batch_ms", tb_prove), ("c_prove_batch_commit_ms", tc)):
                T[key].append(v)
        med = {k: round(statistics.median(v), 2) for k, v in T.items()}
        med["a_total_ms"] = round(statistics.median([x + y for x, y in zip(T["a_commit_ms"], T["a_prove_batch_ms"])]), 2)
        med["b_total_ms"] = round(statistics.median([x + y + z for x, y, z in zip(T["b_commit_ms"], T["b_append_ms"], T["b_prove_batch_ms"])]), 2)
        med["c_total_ms"] = med["c_prove_batch_commit_ms"]
        med["spread_ms"] = {k: [round(min(v), 2), round(max(v), 2)] for k, v in T.items()}
        tmpl.free()
        # the kernels alone, profiled in passes of their own
        ks = []
        fv, fb = [v[32 * j:32 * j + 32] for v in vals for j in range(3)], [b[32 * j:32 * j + 32] for b in blinds for j in range(3)]
        ctx.pedersen_commit(fv, fb)
        for _ in range(a.reps):
            ctx.profile_set(2); ctx.pedersen_commit(fv, fb); r = ctx.profile_report(); ctx.profile_set(0)
            ks.append(r["k_pedersen"]["total_ms"]); assert r["k_pedersen"]["count"] == 1
        kern = {"commitments": 3 * K, "k_pedersen_ms": round(statistics.median(ks), 4), "k_bt_commit_v_ms": {}}
        items = [(vals[k], [], pre, blinds[k], rng(s), 0) for k, s in enumerate(seeds)]
        for cpw in (1, 2, 4):
            os.environ["BPG_COMMIT_CPW"] = str(cpw)
            c2 = context()
            t2 = base.prover.template(c2)
            assert [c for _, _, c in t2.prove_batch_commit(items)] == [k[3] for k in known]
            ks = []
            for _ in range(a.reps):
                c2.profile_set(2); t2.prove_batch_commit(items); r = c2.profile_report(); c2.profile_set(0)
                ks.append(r["k_bt_commit_v"]["total_ms"]); assert r["k_bt_commit_v"]["count"] == 1
            kern["k_bt_commit_v_ms"]["cpw%d" % cpw] = round(statistics.median(ks), 4)
            t2.free(); c2.close()
        del os.environ["BPG_COMMIT_CPW"]
        med["kernels"] = kern
        out["sizes"][str(K)] = med
    print(json.dumps(out, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
