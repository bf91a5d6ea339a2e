#!/usr/bin/env python3
"""What K = 64 depth-8 membership proofs (N = 2^14) of 64 DIFFERENT leaves of one resident 256-leaf tree cost, three ways, in one process:
  (a) gated:      ONE MerklePath256 template (the index in its public inputs) and one prove_batch_inputs of 64 items;
  (b) per_index:  what a tree server could do before gates - one MerkleTree256 template per distinct pattern (host assembly + upload each, the siblings
                  and the root as public inputs) and 64 one-item batches;
  (c) one_index:  the ungated template of ONE index on 64 trees - 64 items of one wave; what gating itself costs per wave is (a) against (c).
Commitments included (commit=True), checkpoints from MerkleTree.path_nodes.  Then verify_batch with per-item inputs against set_inputs + verify per item.
Host clock around synchronised calls; the legs alternate in every repetition (the order rotates); median and min..max of --reps after a warm-up in which
every proof of (a) is verified by the template of (b) for its index.  Beside the times: the launch counts of one pass of (a) and (c) from the engine's
profile (a pass of its own) and what a read-only query says about other work on the card.  Writes one JSON object (profiles/merkle_path_batch.json)."""
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

LABEL = b"MerklePath"
ms = lambda t0: (time.perf_counter() - t0) * 1e3
seed = lambda tag: hashlib.sha256(b"merkle path batch " + tag).digest()


def card_state():
    """what else is on the card, as far as a read-only query tells"""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse", "--showpids", "--json"], capture_output=True, text=True, timeout=20)
        if r.returncode:
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
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_path_batch.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    LC = bpg.LinearCombination
    D, K = a.depth, a.count
    ctx = bpg.Context(0)
    cap = 1 << (1944 * D - 1).bit_length()
    ctx.gens_ensure(cap)
    leaf = lambda t, i: (int.from_bytes(workloads.synth("path-batch-%d" % t, i, 31), "little")).to_bytes(32, "little")
    blind = lambda k: workloads.blinding("path-batch", k)
    tree = ctx.merkle_tree([leaf(0, i) for i in range(1 << D)])
    idx = [(37 * k + 5) % (1 << D) for k in range(K)]
    assert len(set(idx)) == K
    pre = bpg.Transcript(LABEL); bpg.Prover(None, pre); pre = pre.state

    def gated_template():
        t = bpg.Transcript(LABEL); p = bpg.Prover(ctx, t)
        _, var = p.commit(leaf(0, idx[0]), blind(0))
        xs = [p.input(v) for v in tree.path_inputs([idx[0]])[0]]
        bpg.MerklePath256(xs[4 * D], var, [tuple(xs[4 * j:4 * j + 4]) for j in range(D)]).prove(p, [], [])
        return p.template(ctx, checkpoints=[v for v, _, last in p.noted() if last])

    def pattern_of(index):
        pat, order = "W", []
        for k in range(D):
            pat, order = (workloads.hash_pattern("I", pat), [k] + order) if (index >> k) & 1 else (workloads.hash_pattern(pat, "I"), order + [k])
        return pat, order

    def index_template(index, lf, sib, root):
        """MerkleTree256 over the index's pattern, siblings (in the order the gadget consumes them) and root as public inputs -> (template, sibling order)"""
        t = bpg.Transcript(LABEL); p = bpg.Prover(ctx, t)
        _, var = p.commit(lf, blind(0))
        pat, order = pattern_of(index)
        xs = [p.input(sib[k]) for k in order]
        bpg.MerkleTree256(p.input(root), xs, [LC.of(var)], pat).prove(p, [], [])
        return p.template(ctx, checkpoints=[v for v, _, last in p.noted() if last]), order

    T = {}
    note = lambda k, x: T.setdefault(k, []).append(x)

    def leg_gated(keep=None):
        t0 = time.perf_counter()
        tmpl = gated_template(); note("gated_template", ms(t0))
        t1 = time.perf_counter()
        nodes, inputs = tree.path_nodes(idx), tree.path_inputs(idx)
        items = [(leaf(0, i), [], pre, blind(k), seed(b"%d" % k), 0, nodes[k], inputs[k]) for k, i in enumerate(idx)]
        note("gated_read_tree", ms(t1))
        t2 = time.perf_counter()
        res = tmpl.prove_batch_inputs(items, commit=True); note("gated_batch", ms(t2))
        note("gated", ms(t0))
        if keep is not None:
            keep.update(res=res, inputs=inputs, tmpl=tmpl)
        else:
            tmpl.free()

    def leg_per_index(keep=None):
        t0 = time.perf_counter()
        root, paths, nodes = tree.root(), tree.paths(idx), tree.path_nodes(idx)
        out = []
        for k, i in enumerate(idx):
            tmpl, order = index_template(i, leaf(0, i), paths[k], root)
            ins = [paths[k][j] for j in order] + [root]
            out.append(tmpl.prove_batch_inputs([(leaf(0, i), [], pre, blind(k), seed(b"%d" % k), 0, nodes[k], ins)], commit=True)[0])
            if keep is not None:
                keep.setdefault("verdicts", []).append(_verify_with(tmpl, ins, keep["res"][k]))
            tmpl.free()
        note("per_index", ms(t0))
        return out

    def _verify_with(tmpl, ins, r):
        tv = bpg.Transcript(LABEL); v = bpg.Verifier(tv); v.commit(r[2])
        tmpl.set_inputs(ins)
        return tmpl.verify(tv.state, r[2], r[0])

    trees = [tree] + [ctx.merkle_tree([leaf(t, i) for i in range(1 << D)]) for t in range(1, K)]
    one = idx[0]
    one_tmpl, one_order = index_template(one, leaf(0, one), tree.paths([one])[0], tree.root())

    def leg_one_index():
        t0 = time.perf_counter()
        items = []
        for t, tr in enumerate(trees):
            sib, nodes, root = tr.paths([one])[0], tr.path_nodes([one])[0], tr.root()
            items.append((leaf(t, one), [], pre, blind(t), seed(b"%d" % t), 0, nodes, [sib[j] for j in one_order] + [root]))
        note("one_index_read_trees", ms(t0))
        t1 = time.perf_counter()
        res = one_tmpl.prove_batch_inputs(items, commit=True); note("one_index_batch", ms(t1))
        assert all(r[0] is not None for r in res)

    # warm-up: every leg once; every proof of (a) is the statement the per-index template of (b) accepts
    keep = {}
    leg_gated(keep)
    per = leg_per_index(keep)
    leg_one_index()
    assert keep["verdicts"] == [0] * K, keep["verdicts"]
    same_bytes = [r[0] for r in keep["res"]] == [r[0] for r in per]
    T.clear()
    legs = [leg_gated, leg_per_index, leg_one_index]
    before = card_state()
    for rep in range(a.reps):
        for j in range(3):
            legs[(rep + j) % 3]()
    # verification: one call with per-item inputs against set_inputs + verify per item
    tmpl, res, inputs = keep["tmpl"], keep["res"], keep["inputs"]
    states = []
    for r in res:
        tv = bpg.Transcript(LABEL); v = bpg.Verifier(tv); v.commit(r[2]); states.append(tv.state)
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        st, _ = tmpl.verify_batch([(states[k], res[k][2], res[k][0], seed(b"v%d" % k), 0, None, b"".join(inputs[k])) for k in range(K)])
        x = ms(t0)
        t1 = time.perf_counter()
        alone = []
        for k in range(K):
            tmpl.set_inputs(inputs[k]); alone.append(tmpl.verify(states[k], res[k][2], res[k][0], seed(b"v%d" % k)))
        y = ms(t1)
        assert st == alone == [0] * K
        if rep:
            note("verify_batch", x); note("set_inputs_verify_each", y)
    # launch counts of one pass of (a) and of (c), a pass of its own
    counts = {}
    for name, leg in (("gated", leg_gated), ("one_index", leg_one_index)):
        ctx.profile_set(2); leg(); rep = ctx.profile_report(); ctx.profile_set(0)
        counts[name] = {k: v["count"] for k, v in sorted(rep.items())}
    out = {"workload": {"depth": D, "count": K, "n": 1944 * D, "N": cap, "distinct_patterns": len({pattern_of(i)[0] for i in idx})},
           "reps": a.reps, "ms": {k: spread(v[:a.reps]) for k, v in T.items()}, "gated_proofs_equal_per_index_proofs": same_bytes,
           "launches": counts, "card_before": before, "card_after": card_state()}
    tmpl.free(); one_tmpl.free()
    for t in trees:
        t.free()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["ms"], sort_keys=True))


if __name__ == "__main__":
    main()
