#!/usr/bin/env python3
"""Lockstep batch proving against the other two ways of proving the same small items: K sequential Context.prove_flat calls, one
ProverPool(workers=8).prove_batch call and one Context.prove_batch call, for cfg 2 (one 64-bit BOUND, N = 128) and mimc_1_block (N = 1024) at
K in 1, 64, 256, 1024.  Host clock around synchronised calls, warmed up, the three ways alternated in every repetition, median of 5; the bytes
of the three must agree.  Prints one JSON line per row and the whole result last.  --only-batch K: one cfg-2 lockstep batch of K items, warmed and
measured once (the shape for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o pb -- python tools/diag/prove_batch.py --only-batch 256)"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", type=int, default=0)
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import assembly_cases as AC
    ctx = bpg.Context(0)
    ctx.gens_ensure(1 << 14)
    kmax = a.only_batch or max(int(k) for k in a.ks.split(","))

    def cfg2_items():
        out = []
        for k in range(kmax):
            asm = workloads.bounds_check_64(ctx, seed=k)
            inst = asm.prover.instance()
            out.append((inst, asm.transcript.state, inst.v_blinding, hashlib.sha256(b"pb %d" % k).digest(), 0))
        return out

    def mimc_items():
        p, t, _ = AC.build(bpg, "mimc_1_block", ctx)              # one witness, distinct seeds: the same circuit proved K times
        inst = p.instance()
        return [(inst, t.state, inst.v_blinding, hashlib.sha256(b"pb mimc %d" % k).digest(), 0) for k in range(kmax)]

    if a.only_batch:
        items = cfg2_items()
        ctx.prove_batch(items); ctx.prove_batch(items)
        print(json.dumps({"only_batch": a.only_batch}))
        return
    pool = bpg.ProverPool(0, workers=8, gens_capacity=1 << 14)
    out = {"reps": a.reps, "workers": 8, "ms": {}, "proofs_per_s": {}}
    for cname, make in (("cfg2", cfg2_items), ("mimc_1_block", mimc_items)):
        items = make()
        ways = {"sequential": lambda its: [ctx.prove_flat(*it) for it in its], "pool8": pool.prove_batch, "lockstep": ctx.prove_batch}
        for fn in ways.values():
            fn(items[:8])                                           # warm-up
        for k in (int(x) for x in a.ks.split(",")):
            ts = {w: [] for w in ways}
            got = {}
            for _ in range(a.reps):
                for w, fn in ways.items():
                    t0 = time.perf_counter(); got[w] = fn(items[:k]); ts[w].append((time.perf_counter() - t0) * 1e3)
            assert got["sequential"] == got["pool8"] == got["lockstep"], (cname, k)
            row = {w: round(statistics.median(v), 3) for w, v in ts.items()}
            row["lockstep_vs_pool8"] = round(row["pool8"] / row["lockstep"], 2)
            out["ms"]["%s/%d" % (cname, k)] = row
            out["proofs_per_s"]["%s/%d" % (cname, k)] = {w: round(k / row[w] * 1e3, 1) for w in ways}
            print(json.dumps({"circuit": cname, "n": items[0][0].n, "K": k, **row}), flush=True)
    print(json.dumps(out))
    pool.close()
    ctx.close()


if __name__ == "__main__":
    main()
