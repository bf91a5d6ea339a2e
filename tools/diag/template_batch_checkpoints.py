#!/usr/bin/env python3
"""K membership proofs against a resident MiMC Merkle tree proved two ways on one context, warm, generators and tables built: K = --items depth --depth
paths (depth 8: n = 15,552, N = 2^14) at one index of a 2^depth-leaf tree, a fresh witness = the leaf replaced (MerkleTree.update) and what the tree then says
(paths, path_nodes, root).
  (a) ResidentCircuit.prove_batch_checkpointed(commit=True) on the template WITH checkpoints (bpg_r1cs_prove_template_batch_checkpointed): a wave evaluates
      the witnesses in the two levels of the checkpointed schedule;
  (b) ResidentCircuit.prove_batch_commit on the template of the same circuit WITHOUT checkpoints (bpg_r1cs_prove_template_batch_commit): the best way there
      was before - one launch per level of dependent blocks.
Both make the commitments inside the call from the same values, blindings, pre-commit transcript states and seeds, so their results are comparable byte for
byte: they are compared in the warm-up and in every repetition.  Host clock around synchronised calls, (a) and (b) alternated (the order flips every
repetition), median and min..max of --reps.  Then the engine's event profile in passes of their own: launches and summed device time of k_witness_eval_batch
(and of k_witness_ck_verify_batch) per wave, both ways, and what a read-only query says about other work on the card before and after.
Writes one JSON object (profiles/template_batch_checkpoints.json)."""
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

ms = lambda t0: (time.perf_counter() - t0) * 1e3


def card_state():
    """what else is on the card, as far as a read-only query tells: busy and memory percentages, and how many processes have a card open"""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse", "--showpids", "--json"], capture_output=True, text=True, timeout=20)
        if r.returncode != 0:
            return {"unknown": r.stderr[-200:]}
        raw = json.loads(r.stdout)
        cards = {k: {"use_pct": v.get("GPU use (%)"), "vram_pct": v.get("GPU Memory Allocated (VRAM%)")} for k, v in raw.items() if k.startswith("card")}
        return {"cards": cards, "processes_with_a_card_open": len(raw.get("system", {}))}
    except Exception as e:        # no tool, no answer: say so
        return {"unknown": repr(e)}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_batch_checkpoints.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    K, depth = a.items, a.depth
    index = 0x5a5a5 % (1 << depth)
    ctx = bpg.Context(0)
    raw = hashlib.shake_256(b"batch ck path leaves").digest(32 << depth)
    leaves = b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 << depth, 32))     # below 2^252 < l: canonical
    tree = ctx.merkle_tree(leaves)
    pattern, order = workloads.merkle_path_pattern(index, depth)
    rng = lambda k: hashlib.sha256(b"template-batch-checkpoints %d" % k).digest()
    t = bpg.Transcript(b"MerklePath"); bpg.Prover(None, t)
    pre = t.state                                                           # as Prover::new leaves it, before any "V" append

    def fresh(k):
        """witness k from the tree: (values, [-root], pre-commit state, blindings, seed, flags, path nodes)"""
        cfg = "bck-path-%d" % k
        leaf = workloads.synth(cfg, 0, 31) + b"\x07"
        tree.update([index], [leaf])
        sib, root = tree.paths([index])[0], tree.root()
        values = [leaf if what == "leaf" else sib[j] for what, j in order]
        blind = b"".join(workloads.blinding(cfg, i) for i in range(len(values)))
        return (b"".join(values), [bpg.scalar_op("sub", bytes(32), root)], pre, blind, rng(k), 0, tree.path_nodes([index])[0])

    # the two templates, from a prover that assembled witness 0 the existing way
    w0 = fresh(0)
    t0_ = bpg.Transcript(b"MerklePath"); p = bpg.Prover(ctx, t0_)
    vals0 = [w0[0][32 * i:32 * i + 32] for i in range(depth + 1)]
    _, vs = p.commit_many(vals0, [w0[3][32 * i:32 * i + 32] for i in range(depth + 1)])
    bpg.MerkleTree256(tree.root(), [], bpg.vars_to_lc(vs), pattern).prove(p, [], [])
    n = p.get_num_multiplications()
    ctx.gens_ensure(1 << max(n - 1, 1).bit_length())
    rows = [p.num_constraints() - 1]
    ck_vars = [var for var, _, last in p.noted() if last]
    tmpl_ck, tmpl_plain = p.template(ctx, param_rows=rows, checkpoints=ck_vars), p.template(ctx, param_rows=rows)

    t1 = time.perf_counter(); items = [fresh(1 + k) for k in range(K)]; prep = ms(t1)
    plain_items = [it[:6] for it in items]
    ways = {"checkpointed": lambda: tmpl_ck.prove_batch_checkpointed(items, commit=True), "plain": lambda: tmpl_plain.prove_batch_commit(plain_items)}
    want = ways["plain"]()
    assert ways["checkpointed"]() == want, "the checkpointed batch differs from the batch without checkpoints"
    T = {k: [] for k in ways}
    for r in range(a.reps):
        for name in (("checkpointed", "plain") if r % 2 == 0 else ("plain", "checkpointed")):
            t1 = time.perf_counter(); got = ways[name](); T[name].append(ms(t1))
            assert got == want, "repetition %d: %s differs" % (r, name)
    out = {"source_hash": bench.source_hash(), "depth": depth, "index": index, "n": n, "N": 1 << max(n - 1, 1).bit_length(), "items": K, "reps": a.reps,
           "checkpoints_per_item": len(ck_vars), "clock": "host clock around synchronised calls, ms", "ways_alternated": True,
           "proofs_states_commitments_equal": "warm-up and every repetition", "witness_preparation_from_the_tree_ms": round(prep, 3),
           "ms": {k: spread(v) for k, v in T.items()}, "card_before": before}
    out["ms_median_gain"] = round(out["ms"]["plain"]["median"] - out["ms"]["checkpointed"]["median"], 3)
    # the device's share, from the event profile, in passes of their own
    for name, fn in ways.items():
        ctx.profile_set(2)
        fn()
        rep = ctx._report()
        ctx.profile_set(0)
        ev, vf, cv = rep.get("k_witness_eval_batch", {}), rep.get("k_witness_ck_verify_batch", {}), rep.get("k_bt_commit_v", {})
        waves = cv.get("count") or 0                                        # one launch of k_bt_commit_v per wave
        out["profile_" + name] = {"waves": waves, "k_witness_eval_batch_launches": ev.get("count"), "k_witness_eval_batch_ms": ev.get("total_ms"),
                                  "k_witness_eval_batch_launches_per_wave": (ev.get("count") or 0) / waves if waves else None,
                                  "k_witness_eval_batch_ms_per_wave": round((ev.get("total_ms") or 0) / waves, 4) if waves else None,
                                  "k_witness_ck_verify_batch_launches": vf.get("count"), "k_witness_ck_verify_batch_ms": vf.get("total_ms"),
                                  "all_kernels_ms": round(sum(v.get("total_ms", 0) for k, v in rep.items() if isinstance(v, dict) and k.startswith("k_")), 3)}
    out["shared_variants_last"] = ctx.schedule().get("shared_variants_last")
    out["card_after"] = card_state()
    tmpl_ck.free(); tmpl_plain.free(); tree.free(); ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
