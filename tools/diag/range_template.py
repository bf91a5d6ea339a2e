#!/usr/bin/env python3
"""K 64-bit BoundsCheck proofs two ways on one context: through a hinted circuit template (ResidentCircuit.prove_batch: the witnesses are computed on the
device from the committed values) and through what there was before range-proof templates - host assembly of every item, instance export, then
Context.prove_batch.  Both ways make the same Pedersen commitments and transcript states (the host way inside its assembly, the template way alone: `template_commit_ms`);
the totals include them.
Host clock around calls that end synchronised, the two ways alternated in every repetition, median of --reps after one warm-up repetition; the proofs of
the two ways are compared byte for byte in the warm-up.  Then, in passes of their own with the engine's event profile on: the device time of
k_witness_eval_batch for the batch, with the source of a range reduced once per run (WIT_HINT_SAME_SOURCE, the default) and once per bit
(BPG_WIT_HINT_SHARE=0, a packer switch that exists for this measurement).  Prints one JSON object."""
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

    ctx = bpg.Context(0, profile=a.profile) if a.profile else bpg.Context(0)
    ctx.gens_ensure(128)
    rng = lambda k: hashlib.sha256(b"range template %d" % k).digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    lo, hi = bytes(8), b"\xff" * 8

    def commitments(seed):
        """the commitments and the transcript of workloads.bounds_check_64 without its assembly -> (values, blindings, transcript state)"""
        cfg = "cfg2-%d" % seed
        t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
        blinds = [workloads.blinding(cfg, i) for i in range(3)]
        scalars, _, _ = bpg.commit(p, workloads.synth(cfg, 0, 8), blinds[:1])
        _, derived = bpg.BoundsCheck(lo, hi).setup(p, scalars, blinds[1:])
        return b"".join(scalars) + b"".join(d[0] for d in derived), b"".join(blinds), t.state

    base = workloads.bounds_check_64(ctx, seed=0)
    out = {"circuit": "bounds_check_64", "n": base.prover.get_num_multiplications(), "reps": a.reps, "profile": a.profile, "sizes": {}}
    for K in [int(x) for x in a.sizes.split(",")]:
        seeds = list(range(1, K + 1))
        tmpl = base.prover.template(ctx)
        T = {"template_commit_ms": [], "host_commit_and_assemble_ms": [], "host_instance_ms": [], "host_prove_batch_ms": [], "template_prove_batch_ms": []}
        for rep in range(a.reps + 1):
            for way in ((0, 1) if rep % 2 == 0 else (1, 0)):
                if way == 0:
                    t0 = time.perf_counter(); asm = [workloads.bounds_check_64(ctx, seed=s) for s in seeds]; t_asm = ms(t0)
                    t0 = time.perf_counter(); items = [(x.prover.instance(), x.transcript.state) for x in asm]; t_inst = ms(t0)
                    items = [(inst, state, inst.v_blinding, rng(s), 0) for (inst, state), s in zip(items, seeds)]
                    t0 = time.perf_counter(); host = ctx.prove_batch(items); t_prove = ms(t0)
                else:
                    t0 = time.perf_counter(); com = [commitments(s) for s in seeds]; t_com = ms(t0)
                    titems = [(v, [], state, vb, rng(s), 0) for (v, vb, state), s in zip(com, seeds)]
                    t0 = time.perf_counter(); got = tmpl.prove_batch(titems); t_tmpl = ms(t0)
            if rep == 0:
                assert got == host, "the template batch and the host assembly give different proofs"
                continue
            T["template_commit_ms"].append(t_com); T["host_commit_and_assemble_ms"].append(t_asm); T["host_instance_ms"].append(t_inst)
            T["host_prove_batch_ms"].append(t_prove); T["template_prove_batch_ms"].append(t_tmpl)
        med = {k: round(statistics.median(v), 2) for k, v in T.items()}
        med["host_total_ms"] = round(statistics.median([x + y + z for x, y, z in zip(T["host_commit_and_assemble_ms"], T["host_instance_ms"], T["host_prove_batch_ms"])]), 2)
        med["template_total_ms"] = round(statistics.median([x + y for x, y in zip(T["template_commit_ms"], T["template_prove_batch_ms"])]), 2)
        med["spread_ms"] = {k: [round(min(v), 2), round(max(v), 2)] for k, v in T.items()}
        tmpl.free()
        # the evaluation kernel alone, profiled in passes of their own
        for share in ("1", "0"):
            os.environ["BPG_WIT_HINT_SHARE"] = share
            t = base.prover.template(ctx)
            t.prove_batch(titems)
            ks = []
            for _ in range(a.reps):
                ctx.profile_set(2); t.prove_batch(titems); rep_ = ctx.profile_report(); ctx.profile_set(0)
                r = rep_["k_witness_eval_batch"]
                ks.append((r["total_ms"], r["count"]))
            med["k_witness_eval_batch_ms_" + ("shared_source" if share == "1" else "source_per_bit")] = round(statistics.median(x for x, _ in ks), 4)
            med["k_witness_eval_batch_launches"] = ks[0][1]
            t.free()
        del os.environ["BPG_WIT_HINT_SHARE"]
        out["sizes"][str(K)] = med
    print(json.dumps(out, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
