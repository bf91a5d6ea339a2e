#!/usr/bin/env python3
"""MiMC Merkle trees in the prefix layout (Context.merkle_tree(leaves, depth=D, reserve=R)) beside the dense layout and beside the floor arithmetic.

(a) depth 24  build with reserve = leaves against merkle_tree(leaves, depth=24) (the dense layout: a 1 GB array whatever the leaves), 2^10 and 2^20
              leaves, the two alternated.  The same nodes are hashed; the prefix build skips the 1 GB fill.
(b) depth 32  reserve 2^20: the build over 2^20 - 16,384 leaves, append of 1, 64 and 4,096 leaves, update of the same counts, paths of 1,024 indices, and the
              regrow of a 2^19-leaf tree from reserve 2^19 to 2^20 (reserve(2^20): one relayout launch).  Beside every hashing call its floor arithmetic:
              (levels whose parent range fits one block) x the narrow-level floor of profiles/merkle_build.json, the wide levels left to the measurement.
(c) bytes     reserved() of every tree above.
Method: host perf_counter around calls that return synchronised, one warm-up, median and min..max of --reps, legs alternated in one process; then ONE
further call under the engine's event profile for the device time of every hashing launch.  What else is on the card is noted before and after, as far
as a read-only query tells.  Writes one JSON object (kept as profiles/merkle_prefix.json)."""
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
FLOOR_MS = 1.45          # one narrow level: 1,944 dependent products (profiles/merkle_build.json)


def card_state():
    """what else is on the card, as far as a read-only query tells: busy percentage and memory in use before this process opens the device"""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse", "--showpids", "--json"], capture_output=True, text=True, timeout=20)
        return json.loads(r.stdout) if r.returncode == 0 else {"unknown": r.stderr[-200:]}
    except Exception as e:        # no tool, no answer: say so
        return {"unknown": repr(e)}


def narrow_levels(depth, old, new, top=256):
    """levels of growing [old, new) whose parent range fits one block - each costs one floor - and the widths of the others"""
    narrow, wide = 0, []
    for h in range(1, depth + 1):
        count = ((new - 1) >> h) - (old >> h) + 1
        if count > top:
            wide.append(count)
        else:
            narrow += 1
    return narrow, wide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_prefix.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "spread_ms": [round(min(v), 3), round(max(v), 3)], "n": len(v)}

    def leaves_of(tag, n):
        raw = hashlib.shake_256(tag).digest(32 * n)
        return b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 * n, 32))     # below 2^252 < l: canonical

    def profiled(fn):
        ctx.profile_set(2)
        res = fn()
        rep = ctx._report()
        ctx.profile_set(0)
        launches = rep.get("_merkle_launch_ms", [])
        other = {k: round(rep[k]["total_ms"], 4) for k in ("k_mpx_fill", "k_mpx_relayout", "k_merkle_fill_empty", "k_mpx_paths") if k in rep}
        return res, dict(other, launches=[[k, round(v, 4)] for k, v in launches[:64]], launches_sum_ms=round(sum(v for _, v in launches), 3))

    def floors(depth, old, new):
        narrow, wide = narrow_levels(depth, old, new)
        return {"narrow_levels": narrow, "floor_ms": round(narrow * FLOOR_MS, 2), "wide_levels": wide}

    ctx = bpg.Context(0)
    out = {"reps": a.reps,
           "conditions": {"device": "device 0 of the node; card state before this process opened it under card_before", "card_before": before,
                          "host_cpus_usable": len(os.sched_getaffinity(0)),
                          "method": "host perf_counter around calls that end synchronised, one warm-up, median and min..max of reps, legs alternated; "
                                    "launches: HIP-event profile of one further call", "floor_ms_per_narrow_level": FLOOR_MS},
           "depth24": {}, "depth32": {}}

    # ---- (a) depth 24, prefix against dense
    for n in (1 << 10, 1 << 20):
        leaves = leaves_of(b"prefix 24 %d" % n, n)
        ctx.merkle_tree(leaves, depth=24, reserve=n).free()
        ctx.merkle_tree(leaves, depth=24).free()
        P, D, roots, held = [], [], set(), {}
        for r in range(a.reps):
            t0 = time.perf_counter(); t = ctx.merkle_tree(leaves, depth=24, reserve=n); P.append(ms(t0))
            roots.add(t.root()); held["prefix"] = t.reserved; t.free()
            t0 = time.perf_counter(); t = ctx.merkle_tree(leaves, depth=24); D.append(ms(t0))
            roots.add(t.root()); held["dense"] = t.reserved; t.free()
        assert len(roots) == 1, "the two layouts gave different roots"
        t, prof = profiled(lambda: ctx.merkle_tree(leaves, depth=24, reserve=n)); t.free()
        t, prof_d = profiled(lambda: ctx.merkle_tree(leaves, depth=24)); t.free()
        out["depth24"]["%d leaves" % n] = {"prefix": stat(P), "dense": stat(D), "reserved": held, "floors": floors(24, 0, n),
                                           "profile_of_one_prefix_build": prof, "profile_of_one_dense_build": prof_d}
        print("depth 24", n, stat(P), stat(D), held, flush=True)

    # ---- (b) depth 32, reserve 2^20
    depth, reserve, n0 = 32, 1 << 20, (1 << 20) - 16384
    base = leaves_of(b"prefix 32", n0)
    ctx.merkle_tree(base, depth=depth, reserve=reserve).free()
    B = []
    for r in range(a.reps):
        t0 = time.perf_counter(); t = ctx.merkle_tree(base, depth=depth, reserve=reserve); B.append(ms(t0))
        if r < a.reps - 1:
            t.free()
    _, prof = profiled(lambda: ctx.merkle_tree(base, depth=depth, reserve=reserve).free())
    out["depth32"]["build of %d leaves" % n0] = dict(stat(B), floors=floors(depth, 0, n0), reserved=t.reserved, profile_of_one=prof)
    print("depth 32 build", stat(B), t.reserved, flush=True)
    at = n0
    for k in (1, 64, 4096):                                                 # 6 x (1 + 64) and 2 x 4,096 fit the 16,384 free slots with reps <= 5
        reps = a.reps if k < 4096 else 1
        A, U = [], []
        for r in range(reps + 1):                                           # the first pair is the warm-up (kept when there is only one)
            new = leaves_of(b"append %d %d" % (k, r), k)
            t0 = time.perf_counter(); first = t.append(new); ta = ms(t0)
            assert first == at
            t0 = time.perf_counter(); t.update(list(range(at, at + k)), new); tu = ms(t0)
            at += k
            if r or reps == 1:
                A.append(ta); U.append(tu)
        out["depth32"]["%d leaves" % k] = {"append": stat(A), "update": stat(U), "floors": floors(depth, at - k, at)}
        print("depth 32", k, stat(A), stat(U), flush=True)
    assert t.reserved[0] == reserve, "the appends were meant to stay inside the reserve"
    idx = [(i * 2654435761) % (1 << 32) for i in range(1024)]               # anywhere below 2^32: most of them far right of the reserve
    t.paths(idx)
    Pt = []
    for r in range(a.reps):
        t0 = time.perf_counter(); t.paths(idx); Pt.append(ms(t0))
    out["depth32"]["paths of 1024 indices"] = stat(Pt)
    t.free()
    half = leaves_of(b"prefix 32 half", 1 << 19)
    Rg, held = [], None
    for r in range(a.reps + 1):
        t = ctx.merkle_tree(half, depth=depth, reserve=1 << 19)
        root = t.root()
        t0 = time.perf_counter(); t.reserve(1 << 20); tr = ms(t0)
        assert t.root() == root
        held = t.reserved
        t.free()
        if r:
            Rg.append(tr)
    out["depth32"]["regrow 2^19 -> 2^20"] = dict(stat(Rg), reserved_after=held)
    print("depth 32 paths, regrow", stat(Pt), stat(Rg), flush=True)

    out["conditions"]["card_after"] = card_state()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
