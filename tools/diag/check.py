#!/usr/bin/env python3
"""What "is this witness satisfying, and where not" costs on the device (ResidentCircuit.check) against the only way there was before it: prove + verify on
the handle.  Two circuits: the 64-bit BoundsCheck template repeated --items times (1024: n = 131,072; rows of 2, 3, 4 and 65 terms) and the reference's 2^20
instance, the full MiMC Merkle tree of --leaves committed leaves (512: n = 993,384; rows of 2-3 terms), as a flat upload.
Method: host clock around synchronised calls, the ways alternated in every repetition (first check of a fresh handle - with the row-major view -, second
check, prove + verify), median and spread of --reps after a warm-up.  Then the per-kernel event profile of a first and a second check in passes of their own,
and the second check with its row kernels at every --thresholds value (BPG_CHECK_THRESHOLD, a context each).  Whether another proof ran on the device during
the proofs is what the engine itself saw (shared_variants_last).  Prints one JSON object (profiles/check.json)."""
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
rng = lambda k: hashlib.sha256(b"diag-check %d" % k).digest()


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "all": [round(x, 3) for x in xs]}


def profile(ctx, fn):
    ctx.profile_set(2)
    try:
        fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return {k: {"count": v["count"], "device_ms": round(v["total_ms"], 4)} for k, v in rep.items()}


def stub_prover(bpg):
    """an assembly-only prover (hashed stand-in commitments): the template's shape needs no device"""
    class Stub(bpg.Prover):
        def __init__(self, ctx, transcript):
            super().__init__(None, transcript)
            self.test_stub_commitments()
    return Stub


class Repeat:
    """--items BoundsCheck items in one resident repeat; make() gives a FRESH handle with its witness assigned (no view yet)"""
    name = "bounds_check_64_repeat"

    def __init__(self, bpg, workloads, ctx, items):
        self.bpg, self.ctx, self.items = bpg, ctx, items
        self.source = workloads.bounds_check_64(None, seed=1, prover_cls=stub_prover(bpg)).prover
        inst = self.source.instance()
        self.tmpl = self.source.template(ctx)
        self.q_src = inst.q
        self.values = inst.v * items
        self.vb = b"".join(workloads.blinding("diag-check", j) for j in range(inst.m)) * items
        t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
        vs = [self.values[32 * j:32 * j + 32] for j in range(inst.m * items)]
        coms, _ = p.commit_many(vs, [self.vb[32 * j:32 * j + 32] for j in range(len(vs))])
        self.state, self.coms = t.state, b"".join(coms)
        self.n, self.q, self.m = inst.n * items, inst.q * items, inst.m * items

    def make(self):
        rep = self.tmpl.repeat(self.items)
        rep.assign(self.values)
        return rep

    def check(self, h):
        return h.check(None, 16)


class Flat:
    """the reference's 2^20 instance as a flat upload; make() uploads it again"""
    name = "merkle_full_tree"

    def __init__(self, bpg, workloads, ctx, leaves):
        self.ctx = ctx
        a = workloads.merkle_full_tree(ctx, leaves=leaves, seed=None if leaves == 512 else 1)
        self.inst = a.prover.instance()
        self.state, self.coms, self.vb, self.values = a.transcript.state, b"".join(a.commitments), self.inst.v_blinding, self.inst.v
        self.n, self.q, self.m = self.inst.n, self.inst.q, self.inst.m

    def make(self):
        return self.ctx.upload(self.inst)

    def check(self, h):
        return h.check(self.values, 16)


def measure(w, ctx, reps):
    ctx.gens_ensure(1 << max(w.n - 1, 1).bit_length())
    T = {"first_check": [], "second_check": [], "prove": [], "verify": []}
    shared = []
    for k in range(reps + 1):                               # repetition 0 is the warm-up
        h = w.make()
        t0 = time.perf_counter(); r1 = w.check(h); a = ms(t0)
        t0 = time.perf_counter(); r2 = w.check(h); b = ms(t0)
        t0 = time.perf_counter(); proof, _ = h.prove(w.state, w.vb, rng(k)); c = ms(t0)
        shared.append(ctx.schedule()["shared_variants_last"])
        t0 = time.perf_counter(); ok = h.verify(w.state, w.coms, proof, rng(1000 + k)); d = ms(t0)
        assert r1.ok and r2.ok and ok == 0, (r1, r2, ok)
        h.free()
        if k:
            for key, x in zip(T, (a, b, c, d)):
                T[key].append(x)
    out = {"n": w.n, "q": w.q, "m": w.m, "reps": reps, "ms": {k: spread(v) for k, v in T.items()}, "shared_variants_seen": max(shared)}
    pv = statistics.median(T["prove"]) + statistics.median(T["verify"])
    out["prove_plus_verify_ms"] = round(pv, 3)
    out["ratio_to_prove_plus_verify"] = {"first_check": round(pv / statistics.median(T["first_check"]), 1), "second_check": round(pv / statistics.median(T["second_check"]), 1)}
    h = w.make()
    out["profile_first_check"] = profile(ctx, lambda: w.check(h))
    out["profile_second_check"] = profile(ctx, lambda: w.check(h))
    h.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--leaves", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--thresholds", default="32,128,1024")
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    out = {"method": "host clock around synchronised calls, ways alternated per repetition, median/min/max of --reps after one warm-up repetition"}
    ctx = bpg.Context(0)
    out["default_threshold"] = ctx.schedule()["check_threshold"]
    ws = [Repeat(bpg, workloads, ctx, a.items), Flat(bpg, workloads, ctx, a.leaves)]
    for w in ws:
        out[w.name] = measure(w, ctx, a.reps)
    ctx.close()
    # the row kernels at other thresholds: a context each (the knob is read when the context is made), the second check of a handle
    out["thresholds"] = {}
    for th in [int(x) for x in a.thresholds.split(",")]:
        os.environ["BPG_CHECK_THRESHOLD"] = str(th)
        c = bpg.Context(0)
        assert c.schedule()["check_threshold"] == th
        res = {}
        for w in ws:
            w.ctx = c
            if isinstance(w, Repeat):
                w.tmpl = w.source.template(c)
            h = w.make()
            w.check(h)
            wall = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); w.check(h); wall.append(ms(t0))
            p = profile(c, lambda: w.check(h))
            res[w.name] = {"second_check_ms": spread(wall), "k_check_rows_ms": p["k_check_rows"]["device_ms"], "k_check_rows_long_ms": p["k_check_rows_long"]["device_ms"]}
            h.free()
        out["thresholds"][str(th)] = res
        c.close()
    os.environ.pop("BPG_CHECK_THRESHOLD", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
