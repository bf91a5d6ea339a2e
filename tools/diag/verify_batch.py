#!/usr/bin/env python3
"""Batch verification against one verify per proof on the reference's 2^20 circuit (cfg 4): for K in 1, 2, 4, 8, 16 distinct proofs on the resident
upload, K sequential ResidentCircuit.verify calls against ONE Context.verify_batch call.  Host clock around synchronised calls, warmed up, median of
5.  Prints one JSON object.  --only-batch K: just that batch, once warmed and once measured (the shape for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o vb -- python tools/diag/verify_batch.py --only-batch 8)"""
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
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", type=int, default=0)
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    import gen_big_proof_fixtures as GB
    ctx = bpg.Context(0)
    asm = GB.build("cfg4_merkle512", ctx)
    inst, state = asm.prover.instance(), asm.transcript.state
    coms = b"".join(asm.commitments)
    ctx.gens_ensure(1 << 20)
    res = ctx.upload(inst)
    kmax = a.only_batch or max(int(k) for k in a.ks.split(","))
    proofs = [res.prove(state, inst.v_blinding, hashlib.sha256(b"verify batch %d" % k).digest(), 0)[0] for k in range(kmax)]
    seed = bytes(32)

    def batch(k):
        st, _ = ctx.verify_batch([(res, state, coms, p, seed, 0) for p in proofs[:k]], batch_seed=os.urandom(32))
        assert st == [0] * k, st

    def sequential(k):
        for p in proofs[:k]:
            assert res.verify(state, coms, p, seed, 0) == 0

    if a.only_batch:
        batch(a.only_batch); batch(a.only_batch)
        print(json.dumps({"only_batch": a.only_batch}))
        return
    out = {"circuit": "cfg4_merkle512", "n": inst.n, "N": 1 << 20, "reps": a.reps, "ms": {}}
    batch(2); sequential(2)                                          # warm-up
    for k in (int(x) for x in a.ks.split(",")):
        row = {}
        for name, fn in (("sequential", sequential), ("batch", batch)):
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); fn(k); ts.append((time.perf_counter() - t0) * 1e3)
            row[name] = round(statistics.median(ts), 3)
        row["speedup"] = round(row["sequential"] / row["batch"], 2)
        out["ms"][str(k)] = row
        print(json.dumps({"K": k, **row}), flush=True)
    print(json.dumps(out))
    res.free()
    ctx.close()


if __name__ == "__main__":
    main()
