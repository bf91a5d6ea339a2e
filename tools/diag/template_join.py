#!/usr/bin/env python3
"""A mixed statement - --bounds 64-bit bounds checks (n = 128, m = 3 each) AND --paths Merkle paths of depth --depth from a resident tree (n = depth x 1,944
each, the node digests as checkpoints from MerkleTree.path_nodes) - proved three ways on one context, warm, generators and tables built:
  (j) ONE proof of the two templates joined on the device (bpg_r1cs_template_join, made once and timed once): per fresh set of witnesses one Pedersen launch for
      all values, the appends, ResidentCircuit.assign with the checkpoints and ResidentCircuit.prove; then ONE verification on the joined handle;
  (h) the same single proof through the host: every gadget assembled into one Prover (commit, assemble), instance(), upload, prove - the proof bytes must be
      those of (j);
  (s) what a caller does without a host assembly and without the join: repeat(--bounds) and repeat(--paths), two proofs, two verifications.
The three totals (j_total, h_total, s_total) cover the same span, values and blindings to proof(s); the verifications are apart (j_verify, s_verify).
The paths are those of ONE leaf index (one circuit shape) after --paths successive updates of that leaf: every item has a root of its own, which is its
parameter.  Host clock around synchronised calls, the three ways alternated in every repetition (the order rotates), median and min..max of --reps after a
warm-up in which the bytes are compared.  Then the engine's event profile in a pass of its own: the time of each level's launch of one assign on the join, and
beside it the levels of the two parts assigned alone as repeats, --reps profiled passes each.  Writes one JSON object (profiles/template_join.json)."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SEED = hashlib.sha256(b"template join tool").digest()
ms = lambda t0: (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", type=int, default=1024)
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shared-device", choices=["yes", "no", "unknown"], default="unknown", help="was the GPU shared with other work during the run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_join.json"))
    a = ap.parse_args()
    from template_checkpoints import card_state
    before = card_state()
    shared = a.shared_device
    if shared == "unknown" and "cards" in before:           # what the read-only query shows before this process opens the card: others with it open, or a busy card
        busy = any(str(c.get("use_pct")) not in ("0", "None") for c in before["cards"].values())
        shared = "yes" if before["processes_with_a_card_open"] > 0 or busy else "no"
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    B, P, depth = a.bounds, a.paths, a.depth
    n_total = 128 * B + P * depth * 1944
    cap = 1
    while cap < n_total:
        cap *= 2
    ctx = bpg.Context(0)
    ctx.gens_ensure(cap)
    gadget = bpg.BoundsCheck(bytes(8), b"\xff" * 8)
    index = 0x5a5a5 % (1 << depth)
    raw = hashlib.shake_256(b"join tool leaves").digest(32 << depth)
    leaves = b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 << depth, 32))          # below 2^252 < l: canonical
    t0 = time.perf_counter(); tree = ctx.merkle_tree(leaves); tree_build_ms = ms(t0)
    pattern, order = workloads.merkle_path_pattern(index, depth)

    def fresh(k):
        """a fresh set of witnesses: the values and blindings of every item in statement order, the roots, the checkpoint values (and what reading them cost)"""
        w = {"bounds": [], "paths": [], "ck": []}
        for i in range(B):
            cfg = "tj-%d-b%d" % (k, i)
            x = bpg.be_to_scalars(workloads.synth(cfg, 0, 8))
            w["bounds"].append((x + gadget.preprocess(x), [workloads.blinding(cfg, j) for j in range(3)]))
        ck_ms = 0.0
        for i in range(P):
            cfg = "tj-%d-p%d" % (k, i)
            leaf = workloads.synth(cfg, 0, 31) + b"\x07"
            tree.update([index], [leaf])
            sib, root = tree.paths([index])[0], tree.root()
            t1 = time.perf_counter(); w["ck"] += tree.path_nodes([index])[0]; ck_ms += ms(t1)
            w["paths"].append(([leaf if what == "leaf" else sib[j] for what, j in order], [workloads.blinding(cfg, j) for j in range(depth + 1)], root))
        w["checkpoint_read_ms"] = ck_ms
        w["values"] = [v for vs, _ in w["bounds"] for v in vs] + [v for vs, _, _ in w["paths"] for v in vs]
        w["blinds"] = [b for _, bs in w["bounds"] for b in bs] + [b for _, bs, _ in w["paths"] for b in bs]
        w["params"] = [bpg.scalar_op("sub", bytes(32), root) for _, _, root in w["paths"]]
        return w

    def bounds_item(p, vs, bs):
        _, var = p.commit_many(vs, bs)
        gadget.prove(p, var[:1], [(vs[1], var[1]), (vs[2], var[2])])

    def path_item(p, vs, bs, root):
        _, var = p.commit_many(vs, bs)
        bpg.MerkleTree256(root, [], bpg.vars_to_lc(var), pattern).prove(p, [], [])

    def state_before(label):
        t = bpg.Transcript(label)
        bpg.Prover(None, t)
        return t.state

    def appended(state, coms):
        out = C.create_string_buffer(203)
        assert bpg.lib().bpg_test_append_commitments(state, C.c_uint64(len(coms) // 32), coms, out) == 0
        return out.raw[:203]

    # the templates: one item of each kind assembled once
    w0 = fresh(0)
    pb = bpg.Prover(ctx, bpg.Transcript(b"BoundsCheck")); bounds_item(pb, *w0["bounds"][0])
    tb = pb.template(ctx)
    pp = bpg.Prover(ctx, bpg.Transcript(b"MerklePath")); path_item(pp, *w0["paths"][0])
    tp = pp.template(ctx, param_rows=[pp.num_constraints() - 1], checkpoints=[var for var, _, last in pp.noted() if last])
    t1 = time.perf_counter(); joined = ctx.join([(tb, B), (tp, P)]); join_ms = ms(t1)
    t1 = time.perf_counter(); again = ctx.join([(tb, B), (tp, P)]); join_ms_warm = ms(t1)
    again.free()
    rep_b, rep_p = tb.repeat(B), tp.repeat(P)
    assert joined.n == n_total
    pre = {label: state_before(label) for label in (b"MixedStatement", b"BoundsCheck", b"MerklePath")}

    def join_way(w, T):
        t1 = time.perf_counter(); coms = b"".join(ctx.pedersen_commit(w["values"], w["blinds"])); T["j_commit"].append(ms(t1))
        t1 = time.perf_counter(); state = appended(pre[b"MixedStatement"], coms); T["j_append"].append(ms(t1))
        t1 = time.perf_counter(); joined.assign(b"".join(w["values"]), w["params"], checkpoints=w["ck"]); T["j_assign"].append(ms(t1))
        t1 = time.perf_counter(); proof, _ = joined.prove(state, b"".join(w["blinds"]), SEED); T["j_prove"].append(ms(t1))
        T["j_total"].append(sum(T[k][-1] for k in ("j_commit", "j_append", "j_assign", "j_prove")))
        t1 = time.perf_counter(); ok = joined.verify(state, coms, proof); T["j_verify"].append(ms(t1))
        assert ok == 0, "the joined handle rejects its own proof"
        return proof

    def host_way(w, T):
        t = bpg.Transcript(b"MixedStatement"); p = bpg.Prover(ctx, t)
        t1 = time.perf_counter()
        for vs, bs in w["bounds"]:
            bounds_item(p, vs, bs)
        for vs, bs, root in w["paths"]:
            path_item(p, vs, bs, root)
        ta = ms(t1)
        t1 = time.perf_counter(); inst = p.instance(); ti = ms(t1)
        t1 = time.perf_counter(); res = ctx.upload(inst); tu = ms(t1)
        t1 = time.perf_counter(); proof, _ = res.prove(t.state, inst.v_blinding, SEED); tpv = ms(t1)
        res.free()
        for key, v in (("h_commit_and_assemble", ta), ("h_instance", ti), ("h_upload", tu), ("h_prove", tpv), ("h_total", ta + ti + tu + tpv)):
            T[key].append(v)
        return proof

    def separate_way(w, T):
        sizes = []
        for tag, rep, label, items, params, ck in (("s_bounds", rep_b, b"BoundsCheck", w["bounds"], [], None),
                                                    ("s_paths", rep_p, b"MerklePath", [(vs, bs) for vs, bs, _ in w["paths"]], w["params"], w["ck"])):
            values, blinds = [v for vs, _ in items for v in vs], [b for _, bs in items for b in bs]
            t1 = time.perf_counter()
            coms = b"".join(ctx.pedersen_commit(values, blinds))
            state = appended(pre[label], coms)
            rep.assign(b"".join(values), params, checkpoints=ck)
            T[tag + "_commit_assign"].append(ms(t1))
            t1 = time.perf_counter(); proof, _ = rep.prove(state, b"".join(blinds), SEED); T[tag + "_prove"].append(ms(t1))
            t1 = time.perf_counter(); ok = rep.verify(state, coms, proof); T[tag + "_verify"].append(ms(t1))
            assert ok == 0
            sizes.append(len(proof))
        T["s_total"].append(sum(T[k][-1] for k in T if k.endswith("_commit_assign") or (k.startswith("s_") and k.endswith("_prove"))))     # values to proofs, as j_total and h_total
        T["s_verify"].append(T["s_bounds_verify"][-1] + T["s_paths_verify"][-1])
        return sizes

    keys = ("j_commit", "j_append", "j_assign", "j_prove", "j_total", "j_verify", "h_commit_and_assemble", "h_instance", "h_upload", "h_prove", "h_total",
            "s_bounds_commit_assign", "s_bounds_prove", "s_bounds_verify", "s_paths_commit_assign", "s_paths_prove", "s_paths_verify", "s_total", "s_verify")
    warm = {k: [] for k in keys}
    w = fresh(1)
    proof = join_way(w, warm)
    assert host_way(w, warm) == proof, "the join and the host assembly of the conjunction give different proofs"
    sizes = separate_way(w, warm)
    T = {k: [] for k in keys}
    ck_read = []
    ways = (join_way, host_way, separate_way)
    for k in range(a.reps):
        w = fresh(2 + k)
        ck_read.append(w["checkpoint_read_ms"])
        got = {}
        for j in range(3):
            way = ways[(k + j) % 3]
            got[way.__name__] = way(w, T)
        assert got["join_way"] == got["host_way"]
    out = {"source_hash": bench.source_hash(), "bounds": B, "paths": P, "depth": depth, "n_join": n_total, "N_join": cap, "reps": a.reps,
           "shared_device": shared, "shared_device_from": "the caller" if a.shared_device != "unknown" else "the query before the run (card_before)",
           "card_before": before, "ways_alternated": True, "bytes_equal_in_warm_up_and_every_repetition": True,
           "clock": "host clock around synchronised calls, ms", "tree_build_ms": round(tree_build_ms, 3),
           "join_call_ms": {"first": round(join_ms, 3), "second": round(join_ms_warm, 3)},
           "proof_bytes": {"one_proof_of_the_join": len(proof), "bounds_repeat": sizes[0], "paths_repeat": sizes[1]},
           "checkpoint_read_ms": spread(ck_read), "ms": {k: spread(v) for k, v in T.items()}}
    # the device's share of one assign, from the event profile, in a pass of its own: the join, then its two parts alone as repeats
    nb = 3 * B

    def profiled(fn):
        """--reps profiled assigns, one report each: per level the median and min..max of its launch"""
        fn()                                                                    # warm
        names = ("k_witness_eval", "k_witness_eval_repeat", "k_witness_eval_join")
        levels, evals, verifies, launches = [], [], [], set()
        for _ in range(a.reps):
            ctx.profile_set(2)
            fn()
            r = ctx._report()
            ctx.profile_set(0)
            launches.add(sum(r.get(k, {}).get("count", 0) for k in names))
            levels.append(r.get("_witness_launch_ms"))
            evals.append(sum(r.get(k, {}).get("total_ms", 0) for k in names))
            verifies.append(sum(r.get(k, {}).get("total_ms", 0) for k in ("k_witness_ck_verify", "k_witness_ck_verify_join")))
        assert len(launches) == 1 and all(len(l) == len(levels[0]) for l in levels)
        return {"launches": launches.pop(), "passes": a.reps, "level_ms": [spread(list(x)) for x in zip(*levels)], "eval_ms": spread(evals),
                "ck_verify_ms": spread(verifies)}
    values = b"".join(w["values"])
    out["one_assign_profile"] = {
        "join": profiled(lambda: joined.assign(values, w["params"], checkpoints=w["ck"])),
        "bounds_repeat_alone": profiled(lambda: rep_b.assign(values[:32 * nb])),
        "paths_repeat_alone": profiled(lambda: rep_p.assign(values[32 * nb:], w["params"], checkpoints=w["ck"]))}
    out["shared_variants_last"] = ctx.schedule().get("shared_variants_last")
    out["card_after"] = card_state()
    for c in (joined, rep_b, rep_p, tb, tp, tree):
        c.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
