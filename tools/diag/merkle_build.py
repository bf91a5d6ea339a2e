#!/usr/bin/env python3
"""MiMC Merkle trees on the GPU (Context.merkle_tree, MerkleTree.paths / .update) at depth 10, 16 and 20, beside the only way there was before:
the host sponge, one node after the other.

Per depth:
  build_ms         median of --reps builds by host clock around the call (it returns synchronised, and includes the upload of the leaves), after a warm-up;
  launches         the device time of each tree-hashing launch of ONE further build, in launch order, from the engine's event profile (a pass of its own);
  paths_1024_ms    1,024 authentication paths of random leaves, median of --reps;
  update_ms        1, 64 and 4,096 random leaves replaced (distinct indices, fresh ones per repetition), median of --reps - against build_ms, the full rebuild;
and the kernel alone: k_mimc_sponge on 65,536 two-block items, event profile, median of --reps.
(profiles/merkle_constants_ab.json is the run of an earlier form of this tool, when the kernels still came in two forms - constants by wave-uniform loads, or
staged in LDS per block - and every figure was taken both ways; its paths_1024_ms still carry a copy per slice that the binding made then.)
The yardstick: bpg.mimc_sponge (the host's mimc_sponge_1) on 4,096 two-block nodes, timed on the same machine; host_build_ms_scaled is that time per node
times the 2^depth - 1 nodes of a tree - SCALED, not measured.  The root of every build is compared with the host's fold of the same leaves at depth 10.
Writes one JSON object (kept as profiles/merkle_build.json)."""
import argparse
import hashlib
import json
import os
import random
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
    ap.add_argument("--depths", default="10,16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_build.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    med = lambda v: round(statistics.median(v), 3)

    def leaves_of(tag, n):
        raw = hashlib.shake_256(tag).digest(32 * n)
        return b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 * n, 32))     # below 2^252 < l: canonical

    # ---- the yardstick: the host sponge on 4,096 nodes
    nodes = leaves_of(b"host nodes", 2 * 4096)
    bpg.mimc_sponge(nodes[:64])
    t0 = time.perf_counter()
    for i in range(4096):
        bpg.mimc_sponge(nodes[64 * i:64 * i + 64])
    host_ms_4096 = ms(t0)
    out = {"reps": a.reps,
           "conditions": {"device": "device 0 of the node; card state before this process opened it under card_before",
                          "card_before": before, "host_cpus_usable": len(os.sched_getaffinity(0)),
                          "method": "host perf_counter around calls that end synchronised, median of reps after one warm-up; launches: HIP-event profile of one further build"},
           "host": {"nodes": 4096, "total_ms": round(host_ms_4096, 2), "us_per_node": round(host_ms_4096 / 4096 * 1e3, 2)},
           "kernel_alone": {}}
    ctxs = {"gpu": bpg.Context(0)}

    # ---- the kernel alone
    items = leaves_of(b"sponge items", 2 * 65536)
    for name, ctx in ctxs.items():
        got = ctx.mimc_sponge_many(items, 2)
        assert got[0] == bpg.mimc_sponge(items[:64]) and got[-1] == bpg.mimc_sponge(items[-64:])
        ks = []
        for _ in range(a.reps):
            ctx.profile_set(2); ctx.mimc_sponge_many(items, 2); r = ctx.profile_report(); ctx.profile_set(0)
            assert r["k_mimc_sponge"]["count"] == 1
            ks.append(r["k_mimc_sponge"]["total_ms"])
        out["kernel_alone"] = {"k_mimc_sponge_65536x2_ms": med(ks), "spread_ms": [round(min(ks), 3), round(max(ks), 3)]}

    # ---- trees
    out["depths"] = {}
    rnd = random.Random(1)
    for depth in [int(x) for x in a.depths.split(",")]:
        n = 1 << depth
        leaves = leaves_of(b"tree %d" % depth, n)
        rec = {"nodes": n - 1, "host_build_ms_scaled": round(host_ms_4096 / 4096 * (n - 1), 1),
               "host_build_note": "SCALED from the 4,096 host nodes above, not measured"}
        roots = set()
        for name, ctx in ctxs.items():
            ctx.merkle_tree(leaves).free()                                    # warm-up
            T = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); t = ctx.merkle_tree(leaves); T.append(ms(t0))
                roots.add(t.root()); t.free()
            ctx.profile_set(2); t = ctx.merkle_tree(leaves); launches = ctx._report().get("_merkle_launch_ms", []); ctx.profile_set(0)
            r = {"build_ms": med(T), "build_spread_ms": [round(min(T), 3), round(max(T), 3)],
                 "launches": [[k, round(v, 4)] for k, v in launches], "launches_sum_ms": round(sum(v for _, v in launches), 3)}
            idx = [rnd.randrange(n) for _ in range(1024)]
            t.paths(idx)
            T = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); t.paths(idx); T.append(ms(t0))
            r["paths_1024_ms"] = med(T)
            r["update_ms"] = {}
            for k in (1, 64, 4096):
                if k > n:
                    r["update_ms"][str(k)] = None                             # the tree has fewer leaves
                    continue
                new = leaves_of(b"new %d %d" % (depth, k), k)
                t.update(rnd.sample(range(n), k), new)
                T = []
                for _ in range(a.reps):
                    ix = rnd.sample(range(n), k)
                    t0 = time.perf_counter(); t.update(ix, new); T.append(ms(t0))
                r["update_ms"][str(k)] = med(T)
            t.free()
            rec[name] = r
        assert len(roots) == 1, "builds of the same leaves gave different roots"
        if depth <= 10:                                                       # the whole tree on the host is affordable here
            level = [leaves[32 * i:32 * i + 32] for i in range(n)]
            while len(level) > 1:
                level = [bpg.mimc_sponge(level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
            assert roots == {level[0]}, "the device's root differs from the host's"
            rec["root_checked_against_host"] = True
        out["depths"][str(depth)] = rec
    out["conditions"]["card_after"] = card_state()
    for ctx in ctxs.values():
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "conditions"}, indent=1))


if __name__ == "__main__":
    main()
