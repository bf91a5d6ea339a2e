#!/usr/bin/env python3
"""K = --items 64-bit bounds checks (n = 128, m = 3 each) proved three ways on one context, warm, generators and tables built:
  (r) ONE proof of the template repeated K times on the device (bpg_r1cs_template_repeat, made once and timed once): per fresh set of witnesses one
      Pedersen launch for the 3 K values, the appends, ResidentCircuit.assign and ResidentCircuit.prove; then ONE verification on the repeated handle;
  (h) the same single proof through the host: K gadgets assembled into one Prover (commit, assemble), instance(), upload, prove - the proof bytes must be
      those of (r);
  (b) K separate proofs: ONE ResidentCircuit.prove_batch_commit on the template, then ONE Context.verify_batch of the K proofs.
Host clock around synchronised calls, the three ways alternated in every repetition, median and min..max of --reps.  Then the engine's event profile in a
pass of its own: time per launch (= schedule level of the source) of k_witness_eval_repeat for one assign of the repeat, and the same for --chain-items
copies of the Merkle pattern ((W W) W), whose lanes are chains of 972 and 1,944 dependent products.  Writes one JSON object (profiles/template_repeat.json)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain-items", type=int, default=256, help="items of the Merkle ((W W) W) repeat whose assign is profiled per level")
    ap.add_argument("--shared-device", choices=["yes", "no", "unknown"], default="unknown", help="was the GPU shared with other work during the run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_repeat.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    K = a.items
    lo, hi = bytes(8), b"\xff" * 8
    n_total = 128 * K
    cap = 1
    while cap < n_total:
        cap *= 2
    ctx = bpg.Context(0)
    ctx.gens_ensure(cap)
    seed = hashlib.sha256(b"template-repeat").digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    gadget = bpg.BoundsCheck(lo, hi)

    def witness(k):
        cfg = "tr-%d" % k
        w = bpg.be_to_scalars(workloads.synth(cfg, 0, 8))
        return w + gadget.preprocess(w), [workloads.blinding(cfg, i) for i in range(3)]

    ws = [witness(k) for k in range(K)]
    values = [v for vs, _ in ws for v in vs]
    blinds = [b for _, bs in ws for b in bs]

    def state_before():
        t = bpg.Transcript(b"BoundsCheck")
        bpg.Prover(None, t)
        return t.state

    def appended(state, coms):
        out = C.create_string_buffer(203)
        assert bpg.lib().bpg_test_append_commitments(state, C.c_uint64(len(coms) // 32), coms, out) == 0
        return out.raw[:203]

    pre = state_before()
    # the template: one item assembled once
    t0 = bpg.Transcript(b"BoundsCheck"); p0 = bpg.Prover(ctx, t0)
    _, vs0 = p0.commit_many(ws[0][0], ws[0][1])
    gadget.prove(p0, vs0[:1], [(ws[0][0][1], vs0[1]), (ws[0][0][2], vs0[2])])
    tmpl = p0.template(ctx)
    t1 = time.perf_counter(); rep = tmpl.repeat(K); repeat_ms = ms(t1)
    t1 = time.perf_counter(); rep2 = tmpl.repeat(K); repeat_ms_warm = ms(t1)
    rep2.free()

    def repeat_way(T):
        t1 = time.perf_counter(); coms = b"".join(ctx.pedersen_commit(values, blinds)); T["r_commit"].append(ms(t1))
        t1 = time.perf_counter(); state = appended(pre, coms); T["r_append"].append(ms(t1))
        t1 = time.perf_counter(); rep.assign(b"".join(values)); T["r_assign"].append(ms(t1))
        t1 = time.perf_counter(); proof, _ = rep.prove(state, b"".join(blinds), seed); T["r_prove"].append(ms(t1))
        T["r_total"].append(sum(T[k][-1] for k in ("r_commit", "r_append", "r_assign", "r_prove")))
        t1 = time.perf_counter(); ok = rep.verify(state, coms, proof); T["r_verify"].append(ms(t1))
        assert ok == 0, "the repeated handle rejects its own proof"
        return proof

    def host_way(T):
        t = bpg.Transcript(b"BoundsCheck"); p = bpg.Prover(ctx, t)
        tc = ta = 0.0
        for vs, bs in ws:
            t1 = time.perf_counter(); _, var = p.commit_many(vs, bs); tc += ms(t1)
            t1 = time.perf_counter(); gadget.prove(p, var[:1], [(vs[1], var[1]), (vs[2], var[2])]); ta += ms(t1)
        t1 = time.perf_counter(); inst = p.instance(); ti = ms(t1)
        t1 = time.perf_counter(); res = ctx.upload(inst); tu = ms(t1)
        t1 = time.perf_counter(); proof, _ = res.prove(t.state, inst.v_blinding, seed); tp = ms(t1)
        res.free()
        for key, v in (("h_commit", tc), ("h_assemble", ta), ("h_instance", ti), ("h_upload", tu), ("h_prove", tp), ("h_total", tc + ta + ti + tu + tp)):
            T[key].append(v)
        return proof

    def batch_way(T):
        items = [(b"".join(vs), [], pre, b"".join(bs), seed, 0) for vs, bs in ws]
        t1 = time.perf_counter(); res = tmpl.prove_batch_commit(items); T["b_prove_batch_commit"].append(ms(t1))
        vitems = [(tmpl, appended(pre, coms), coms, proof) for proof, _, coms in res]
        t1 = time.perf_counter(); st, _ = ctx.verify_batch(vitems); T["b_verify_batch"].append(ms(t1))
        assert st == [0] * K
        return sum(len(proof) for proof, _, _ in res)

    keys = ("r_commit", "r_append", "r_assign", "r_prove", "r_total", "r_verify", "h_commit", "h_assemble", "h_instance", "h_upload", "h_prove", "h_total",
            "b_prove_batch_commit", "b_verify_batch")
    warm = {k: [] for k in keys}
    proof = repeat_way(warm)
    assert host_way(warm) == proof, "the repeat and the host assembly of the K-fold circuit give different proofs"
    batch_bytes = batch_way(warm)
    T = {k: [] for k in keys}
    for _ in range(a.reps):
        proof = repeat_way(T)
        assert host_way(T) == proof
        batch_way(T)
    out = {"source_hash": bench.source_hash(), "items": K, "n_item": 128, "n_repeat": n_total, "N_repeat": cap, "reps": a.reps, "shared_device": a.shared_device,
           "repeat_call_ms": {"first": round(repeat_ms, 3), "second": round(repeat_ms_warm, 3)},
           "proof_bytes": {"one_proof_of_the_repeat": len(proof), "separate_proofs_total": batch_bytes},
           "ms_median": {k: round(statistics.median(v), 3) for k, v in T.items()},
           "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in T.items()}}
    ctx.profile_set(2)
    rep.assign(b"".join(values))
    r = ctx._report()
    ctx.profile_set(0)
    k = r.get("k_witness_eval_repeat", {})
    out["k_witness_eval_repeat_one_assign"] = {"launches": k.get("count"), "device_ms": k.get("total_ms"), "level_ms": r.get("_witness_launch_ms")}
    rep.free(); tmpl.free()
    # ... and for lanes that are latency chains (972 dependent products each): the Merkle pattern ((W W) W) (n = 3,888: four absorbed blocks in three segments, one per level)
    # repeated --chain-items times, assign alone (no proof: the evaluation needs no generators) beside one assign of the template itself
    t0 = bpg.Transcript(b"MerkleTree"); p0 = bpg.Prover(ctx, t0)
    leaves = lambda k: [b"\x03" + workloads.synth("tr-mk-%d" % k, i, 31) for i in range(3)]
    _, _, vs0 = bpg.commit_all_single(p0, leaves(0), [workloads.blinding("tr-mk", i) for i in range(3)])
    bpg.MerkleTree256(bytes(32), [], bpg.vars_to_lc(vs0), "((W W) W)").prove(p0, [], [])
    tmpl = p0.template(ctx, param_rows=[p0.num_constraints() - 1])
    KC = a.chain_items
    rep = tmpl.repeat(KC)
    chain_values = b"".join(bpg.be_to_scalar(x) for k in range(KC) for x in leaves(k))
    chain = {}
    for name, c, v, params in (("repeat", rep, chain_values, [bytes(32)] * KC), ("template_alone", tmpl, chain_values[:96], [bytes(32)])):
        c.assign(v, params)                                                 # warm
        ctx.profile_set(2)
        c.assign(v, params)
        r = ctx._report()
        ctx.profile_set(0)
        chain[name] = {"launches": sum(r.get(k, {}).get("count", 0) for k in ("k_witness_eval", "k_witness_eval_repeat")), "level_ms": r.get("_witness_launch_ms")}
    out["merkle3_chain_lanes"] = {"items": KC, "n_repeat": rep.n, "assign": chain}
    rep.free(); tmpl.free(); ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
