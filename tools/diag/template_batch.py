#!/usr/bin/env python3
"""K fresh witnesses of the 8-leaf MiMC Merkle tree (n = 13,608, N = 2^14) proved two ways on one context, warm, generators and tables built:
  (a) host assembly of the K instances (the gadget's prove() call and instance(), timed apart) + one Context.prove_batch (bpg_r1cs_prove_batch);
  (b) one ResidentCircuit.prove_batch on the template (bpg_r1cs_prove_template_batch): the witnesses are computed on the device.
The leaf commitments are common to both ways and timed apart.  Host clock around synchronised calls, (a) and (b) alternated in every repetition, median and
min..max of --reps; every proof of (b) is compared with (a)'s.  Then the engine's event profile, in passes of their own: time per launch (= level) of
k_witness_eval_batch at K = 1, 8 and --items, and of k_witness_eval for one assign.  Writes one JSON object (profiles/template_batch.json)."""
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
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shared-device", choices=["yes", "no", "unknown"], default="unknown", help="was the GPU shared with other work during the run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_batch.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    L, K, LEAVES = bpg.L, a.items, 8
    ctx = bpg.Context(0)
    ctx.gens_ensure(1 << 14)
    pattern = workloads.full_tree_pattern(LEAVES)
    rng = lambda k: hashlib.sha256(b"template-batch %d" % k).digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3

    def witness(seed):
        cfg = "tb-%d" % seed
        leaf_be = [b"\x07" + workloads.synth(cfg, i, 31) for i in range(LEAVES)]
        probe = bpg.Prover(None, bpg.Transcript(b"probe"))                 # the root is an input of a real prover; this stands in for knowing it
        bpg.MerkleTree256(bytes(32), [bpg.be_to_scalar(b) for b in leaf_be], [], pattern.replace("W", "I")).prove(probe, [], [])
        return leaf_be, [workloads.blinding(cfg, i) for i in range(LEAVES)], probe.instance().aO[-32:]

    ws = [witness(s) for s in range(K)]

    def host_way(T):
        """commit, assemble, flatten every witness, then ONE prove_batch"""
        items, tc, ta, ti = [], 0.0, 0.0, 0.0
        for k, (leaf_be, blind, root) in enumerate(ws):
            t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
            t0 = time.perf_counter(); _, _, wvars = bpg.commit_all_single(p, leaf_be, blind); tc += ms(t0)
            t0 = time.perf_counter(); bpg.MerkleTree256(root, [], bpg.vars_to_lc(wvars), pattern).prove(p, [], []); ta += ms(t0)
            t0 = time.perf_counter(); inst = p.instance(); ti += ms(t0)
            items.append((inst, t.state, inst.v_blinding, rng(k), 0))
        t0 = time.perf_counter(); res = ctx.prove_batch(items); tp = ms(t0)
        for key, v in (("commit", tc), ("assemble", ta), ("instance", ti), ("prove_batch", tp), ("host_way_without_commit", ta + ti + tp)):
            T[key].append(v)
        return res, items[0][0], p

    def template_way(tmpl, T, count=None):
        """commit (for the transcript), then ONE template batch"""
        items, tc = [], 0.0
        for k, (leaf_be, blind, root) in enumerate(ws[:count]):
            t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
            t0 = time.perf_counter(); bpg.commit_all_single(p, leaf_be, blind); tc += ms(t0)
            v = b"".join(bpg.be_to_scalar(b) for b in leaf_be)
            minus_root = ((L - int.from_bytes(root, "little")) % L).to_bytes(32, "little")
            items.append((v, [minus_root], t.state, b"".join(blind), rng(k), 0))
        t0 = time.perf_counter(); res = tmpl.prove_batch(items); tp = ms(t0)
        T["commit_t"].append(tc); T["prove_template_batch"].append(tp)
        return res

    keys = ("commit", "assemble", "instance", "prove_batch", "host_way_without_commit", "commit_t", "prove_template_batch")
    warm = {k: [] for k in keys}
    want, inst0, p0 = host_way(warm)
    tmpl = p0.template(ctx, param_rows=[p0.num_constraints() - 1])
    assert template_way(tmpl, warm) == want, "the template batch differs from the host assembly's proofs"
    T = {k: [] for k in keys}
    for _ in range(a.reps):
        want, _, _ = host_way(T)
        assert template_way(tmpl, T) == want, "the template batch differs from the host assembly's proofs"
    out = {"source_hash": bench.source_hash(), "leaves": LEAVES, "n": inst0.n, "items": K, "reps": a.reps, "shared_device": a.shared_device,
           "ms_median": {k: round(statistics.median(v), 3) for k, v in T.items()},
           "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in T.items()}}
    # device time of the evaluation alone (event profile, passes of their own)
    levels = {}
    for count in sorted({1, 8, K}):
        ctx.profile_set(2)
        template_way(tmpl, {k: [] for k in keys}, count)
        rep = ctx._report()
        ctx.profile_set(0)
        k = rep.get("k_witness_eval_batch", {})
        levels[str(count)] = {"launches": k.get("count"), "device_ms": k.get("total_ms"),
                              "ms_per_launch": round(k["total_ms"] / k["count"], 4) if k.get("count") else None}
    out["k_witness_eval_batch"] = levels
    leaf_be, blind, root = ws[0]
    ctx.profile_set(2)
    tmpl.assign(b"".join(bpg.be_to_scalar(b) for b in leaf_be), [((L - int.from_bytes(root, "little")) % L).to_bytes(32, "little")])
    rep = ctx._report()
    ctx.profile_set(0)
    k = rep.get("k_witness_eval", {})
    out["k_witness_eval_single_assign"] = {"launches": k.get("count"), "device_ms": k.get("total_ms"), "level_ms": rep.get("_witness_launch_ms")}
    tmpl.free(); ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
