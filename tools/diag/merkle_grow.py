#!/usr/bin/env python3
"""Growing MiMC Merkle trees (Context.merkle_tree(leaves, depth=D), MerkleTree.append) beside what a caller did before them.

(a) build    merkle_tree(leaves, depth=D) against padding the leaf list to 2^D on the host and calling the full build (the padding itself is timed too:
             it is part of what the caller did).  D = 20 with 2^10, 2^16 and 2^20 - 1 leaves; D = 24 with 2^10 and 2^20 leaves, the padded leg ONCE only
             (it uploads 512 MB and hashes 2^24 nodes).
(b) append   append of 1, 64 and 4,096 leaves against update of the same indices with the same leaves, at D = 20 on two trees of identical content: both
             start from 2^19 leaves; the update leg's tree counts the slots the appends will fill as leaves that hold the empty value already, so the two
             trees are node for node the same before and after every pair of calls (the roots are compared every time).
Method: host perf_counter around calls that return synchronised, one warm-up, median and min..max of --reps, the two ways alternated in one process; then
ONE further call of each new way under the engine's event profile for the device time of every launch, in launch order.  What else is on the card is noted
before and after, as far as a read-only query tells.  Writes one JSON object (kept as profiles/merkle_grow.json)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def card_state():
    """what else is on the card, as far as a read-only query tells: busy percentage and memory in use before this process opens the device"""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse", "--showpids", "--json"], capture_output=True, text=True, timeout=20)
        return json.loads(r.stdout) if r.returncode == 0 else {"unknown": r.stderr[-200:]}
    except Exception as e:        # no tool, no answer: say so
        return {"unknown": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-depth24", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_grow.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "spread_ms": [round(min(v), 3), round(max(v), 3)], "n": len(v)}

    def leaves_of(tag, n):
        raw = hashlib.shake_256(tag).digest(32 * n)
        return b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 * n, 32))     # below 2^252 < l: canonical

    def profiled(fn):
        """fn() under the event profile -> the device time of the fill and of every hashing launch, in launch order"""
        ctx.profile_set(2)
        res = fn()
        rep = ctx._report()
        ctx.profile_set(0)
        launches = rep.get("_merkle_launch_ms", [])
        return res, {"k_merkle_fill_empty_ms": round(rep.get("k_merkle_fill_empty", {}).get("total_ms", 0.0), 4),
                     "launches": [[k, round(v, 4)] for k, v in launches], "launches_sum_ms": round(sum(v for _, v in launches), 3)}

    ctx = bpg.Context(0)
    out = {"reps": a.reps,
           "conditions": {"device": "device 0 of the node; card state before this process opened it under card_before", "card_before": before,
                          "host_cpus_usable": len(os.sched_getaffinity(0)),
                          "method": "host perf_counter around calls that end synchronised, one warm-up, median and min..max of reps, the two ways alternated; "
                                    "launches: HIP-event profile of one further call"},
           "build": {}, "append": {}}

    # ---- (a) build
    def padded_build(leaves, depth):
        t0 = time.perf_counter()
        data = leaves + bytes(32 * (1 << depth) - len(leaves))              # what the caller does today: pad on the host ...
        pad_ms = ms(t0)
        t = ctx.merkle_tree(data)                                           # ... and upload and hash all of it
        return t, ms(t0), pad_ms

    cases = [(20, 1 << 10), (20, 1 << 16), (20, (1 << 20) - 1)] + ([] if a.skip_depth24 else [(24, 1 << 10), (24, 1 << 20)])
    for depth, n in cases:
        leaves = leaves_of(b"grow %d %d" % (depth, n), n)
        padded_reps = a.reps if depth < 24 else 1
        ctx.merkle_tree(leaves, depth=depth).free()                         # warm-up of the new way (allocates and frees the array once)
        if depth < 24:
            padded_build(leaves, depth)[0].free()
        G, P, PAD, roots = [], [], [], set()
        for r in range(a.reps):
            t0 = time.perf_counter(); t = ctx.merkle_tree(leaves, depth=depth); G.append(ms(t0))
            roots.add(t.root()); t.free()
            if r < padded_reps:
                t, total, pad = padded_build(leaves, depth)
                P.append(total); PAD.append(pad)
                roots.add(t.root()); t.free()
        assert len(roots) == 1, "the grown build and the padded build gave different roots"
        t, prof = profiled(lambda: ctx.merkle_tree(leaves, depth=depth))
        t.free()
        out["build"]["depth %d, %d leaves" % (depth, n)] = {
            "grow": stat(G), "padded": dict(stat(P), host_padding_ms_median=round(statistics.median(PAD), 3),
                                            note="no warm-up, one run" if depth == 24 else "after one warm-up"),
            "array_mb": (64 << depth) >> 20, "profile_of_one_grow": prof}
        print("build", depth, n, out["build"]["depth %d, %d leaves" % (depth, n)]["grow"], out["build"]["depth %d, %d leaves" % (depth, n)]["padded"], flush=True)

    # ---- (b) append against update of the same indices
    depth, n0 = 20, 1 << 19
    base = leaves_of(b"append base", n0)
    for k in (1, 64, 4096):
        room = k * (a.reps + 2)
        grown = ctx.merkle_tree(base, depth=depth)
        other = ctx.merkle_tree(base + bytes(32 * room), depth=depth)       # the same nodes: the slots to come hold the empty value (zero) as leaves
        assert grown.root() == other.root()
        A, U = [], []
        for r in range(a.reps + 1):                                         # the first pair is the warm-up
            new = leaves_of(b"append %d %d" % (k, r), k)
            at = n0 + r * k
            t0 = time.perf_counter(); first = grown.append(new); ta = ms(t0)
            t0 = time.perf_counter(); other.update(list(range(at, at + k)), new); tu = ms(t0)
            assert first == at and grown.root() == other.root()
            if r:
                A.append(ta); U.append(tu)
        _, prof = profiled(lambda: grown.append(leaves_of(b"append %d last" % k, k)))
        grown.free(); other.free()
        out["append"]["%d leaves" % k] = {"append": stat(A), "update": stat(U), "profile_of_one_append": prof}
        print("append", k, out["append"]["%d leaves" % k]["append"], out["append"]["%d leaves" % k]["update"], flush=True)

    out["conditions"]["card_after"] = card_state()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
