#!/usr/bin/env python3
"""Keyed MiMC Merkle trees (Context.merkle_tree(leaves, depth=D, keys=[...])) beside the prefix layout of the same leaves.

(a) build    2^10, 2^16 and 2^20 keys at depths 24 and 32, with random keys and with the consecutive keys 0 .. n-1, and beside each the prefix-layout build
             (reserve = n) of the same leaves at the same depth, the two alternated.  With consecutive keys the two trees are the same tree, node for node
             (the roots are compared); with random keys the keyed tree hashes about n (D - lg n + 2) nodes where the prefix tree hashes 2n.
(b) put      1, 64 and 4,096 new random keys into a depth-32 tree of 2^20 random keys.
(c) paths    of 4,096 keys, half of them held, on that tree.
(d) counts   node_counts of every tree above: stored nodes per height and the bytes held.
Method: host perf_counter around the C calls (ctypes arrays made beforehand), which return synchronised; one warm-up, median and min..max of --reps, legs
alternated in one process; then ONE further call under the engine's event profile for the device time of every kernel of the put.  The host's sort of the
keys is inside the timed call: it is part of a put.  Writes one JSON object (kept as profiles/merkle_keyed.json)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KEYED_KERNELS = ("k_mkx_classify", "k_mkx_scan_sums", "k_mkx_scan_top", "k_mkx_scatter", "k_mkx_merge", "k_mkx_set_leaves", "k_mkx_level", "k_mkx_climb", "k_mkx_paths")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-lg", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_keyed.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    lib = bpg.lib()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "spread_ms": [round(min(v), 3), round(max(v), 3)], "n": len(v)}

    def leaves_of(tag, n):
        raw = hashlib.shake_256(tag).digest(32 * n)
        return b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 * n, 32))     # below 2^252 < l: canonical

    def keys_of(tag, n, depth, avoid=()):
        """n distinct seeded keys below 2^depth, unsorted"""
        out, seen, i = [], set(avoid), 0
        while len(out) < n:
            raw = hashlib.shake_256(tag + b"%d" % i).digest(8 * max(n, 64))
            for k in range(0, len(raw), 8):
                v = int.from_bytes(raw[k:k + 8], "little") >> (64 - depth)
                if v not in seen:
                    seen.add(v); out.append(v)
                    if len(out) == n:
                        break
            i += 1
        return out

    class Tree(bpg.MerkleTree):
        """a handle made by a timed C call, served by the package's methods afterwards"""
        def __init__(self, ctx, depth, handle, keyed):
            self.ctx, self.depth, self._h, self.keyed = ctx, depth, handle, keyed

    def build_keyed(depth, n, karr, leaves):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.bpg_merkle_build_keyed(ctx._h, C.c_uint32(depth), C.c_uint64(n), karr, leaves, None, C.byref(h))
        t = ms(t0)
        assert rc == 0, rc
        return Tree(ctx, depth, h, True), t

    def build_prefix(depth, n, leaves):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.bpg_merkle_build_prefix(ctx._h, C.c_uint32(depth), C.c_uint64(n), C.c_uint64(n), leaves, None, C.byref(h))
        t = ms(t0)
        assert rc == 0, rc
        return Tree(ctx, depth, h, False), t

    def profiled(fn):
        ctx.profile_set(2)
        res = fn()
        rep = ctx._report()
        ctx.profile_set(0)
        kernels = {k: {"count": rep[k]["count"], "total_ms": round(rep[k]["total_ms"], 4), "nodes": int(rep[k]["field_mults"] // 1944)} for k in KEYED_KERNELS if k in rep}
        return res, {"kernels": kernels, "device_ms": round(sum(v["total_ms"] for v in kernels.values()), 3),
                     "hashing_launches": [[k, round(v, 4)] for k, v in rep.get("_merkle_launch_ms", [])[:40]]}

    ctx = bpg.Context(0)
    out = {"reps": a.reps,
           "conditions": {"device": "device 0 of the node", "host_cpus_usable": len(os.sched_getaffinity(0)),
                          "method": "host perf_counter around C calls that end synchronised (the host's key sort included), one warm-up, median and min..max of "
                                    "reps, keyed and prefix legs alternated; kernels: HIP-event profile of one further call"},
           "build": {}, "put": {}, "paths": {}}

    # ---- (a) builds, keyed beside prefix
    big = None
    for depth in (24, 32):
        for lg in (10, 16, 20):
            if lg > a.max_lg:
                continue
            n = 1 << lg
            leaves = leaves_of(b"keyed %d %d" % (depth, n), n)
            for kind in ("random", "consecutive"):
                keys = keys_of(b"keyed build %d %d" % (depth, n), n, depth) if kind == "random" else list(range(n))
                karr = (C.c_uint64 * n)(*keys)
                t, _ = build_keyed(depth, n, karr, leaves); t.free()
                t, _ = build_prefix(depth, n, leaves); t.free()
                Kt, Pt, counts, held_p, roots = [], [], None, None, set()
                for r in range(a.reps):
                    t, dt = build_keyed(depth, n, karr, leaves); Kt.append(dt)
                    counts = t.node_counts
                    roots.add(t.root()); t.free()
                    t, dt = build_prefix(depth, n, leaves); Pt.append(dt)
                    held_p = t.reserved
                    if kind == "consecutive":
                        roots.add(t.root())
                    t.free()
                assert len(roots) == 1, "a consecutive-key tree and the prefix tree of the same leaves gave different roots"
                (t, _), prof = profiled(lambda: build_keyed(depth, n, karr, leaves))
                name = "depth %d, 2^%d %s keys" % (depth, lg, kind)
                out["build"][name] = {"keyed": stat(Kt), "prefix_same_leaves": stat(Pt), "stored_nodes": sum(counts[0]), "node_counts": counts[0], "keyed_bytes": counts[1],
                                      "prefix_bytes": held_p[1], "nodes_hashed": sum(v["nodes"] for v in prof["kernels"].values()), "profile_of_one_keyed_build": prof}
                print(name, stat(Kt), stat(Pt), sum(counts[0]), flush=True)
                if depth == 32 and kind == "random" and lg == min(20, a.max_lg):
                    big, big_keys = t, keys
                else:
                    t.free()

    # ---- (b) puts of new keys into the big tree, (c) paths
    depth, have = 32, set(big_keys)
    for k in (1, 64, 4096):
        T, prof = [], None
        for r in range(a.reps + 2):                                         # the first is the warm-up, the last runs under the profile
            new = keys_of(b"put %d %d" % (k, r), k, depth, have)
            have.update(new)
            karr, leaves = (C.c_uint64 * k)(*new), leaves_of(b"put leaves %d %d" % (k, r), k)
            ins = C.c_uint64()

            def call():
                t0 = time.perf_counter()
                rc = lib.bpg_merkle_put(ctx._h, big._h, C.c_uint64(k), karr, leaves, C.byref(ins), None)
                assert rc == 0 and ins.value == k, (rc, ins.value)
                return ms(t0)
            if r == a.reps + 1:
                _, prof = profiled(call)
            elif r:
                T.append(call())
            else:
                call()
        out["put"]["%d new keys into 2^%d" % (k, min(20, a.max_lg))] = dict(stat(T), profile_of_one=prof)
        print("put", k, stat(T), flush=True)
    held = sorted(have)
    idx = [held[(i * 2654435761) % len(held)] for i in range(2048)] + [(i * 2654435761 + 12345) % (1 << 32) for i in range(2048)]
    big.paths(idx)
    Pt = []
    for r in range(a.reps):
        t0 = time.perf_counter(); big.paths(idx); Pt.append(ms(t0))
    out["paths"]["4096 keys, half of them held"] = stat(Pt)
    out["paths"]["node_counts_of_the_tree"] = big.node_counts
    print("paths", stat(Pt), flush=True)
    big.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
