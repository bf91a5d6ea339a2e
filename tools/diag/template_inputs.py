#!/usr/bin/env python3
"""--items LessThan proofs (n = 379, N = 512) against as many DIFFERENT public bounds, proved two ways on one context, warm, generators and tables built:
  (a) one ResidentCircuit.prove_batch_inputs(commit=True) on ONE template whose bound is a public input (bpg_r1cs_prove_template_batch_inputs): every item
      brings its committed values, blindings and its bound;
  (b) the best way there was before public inputs: a host assembly per bound with the bound baked in as a constant (Prover, three commitments in one deferred
      launch, LessThan through the gadget surface), the flattened instance, then ONE bpg_r1cs_prove_batch over all of them.  The assembly runs through the
      Python bindings, as a Python service would run it; its share is reported apart.
Both make the Pedersen commitments inside the timed region from the same values, blindings and seeds, so the results are comparable byte for byte: proofs,
commitments and transcript states are compared in the warm-up and in every repetition.  Host clock around synchronised calls, (a) and (b) alternated (the
order flips every repetition), median and min..max of --reps; what a read-only query says about other work on the card before and after.
Writes one JSON object (profiles/template_inputs.json)."""
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
sc = lambda x: x.to_bytes(32, "little")


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_inputs.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    import bench
    K = a.items
    L = bpg.L
    ctx = bpg.Context(0)
    ctx.gens_ensure(512)
    rng = lambda k: hashlib.sha256(b"template-inputs %d" % k).digest()
    t = bpg.Transcript(b"LessThan"); bpg.Prover(None, t)
    pre = t.state                                                           # as Prover::new leaves it, before any "V" append

    # statement k: left_k < bound_k, every bound different; the committed values are (left, delta, delta^-1), as LessThan::setup derives them
    def statement(k):
        cfg = "template-inputs-%d" % k
        bound = int.from_bytes(workloads.synth(cfg, 0, 15), "big") | (1 << 64) | k
        left = int.from_bytes(workloads.synth(cfg, 1, 15), "big") % bound
        delta = bound - left
        values = [sc(left), sc(delta), sc(pow(delta, L - 2, L))]
        return bound, values, [workloads.blinding(cfg, i) for i in range(3)]
    stmts = [statement(k) for k in range(K)]
    assert len({b for b, _, _ in stmts}) == K

    def assemble(bound, values, blinds, as_input):
        tr = bpg.Transcript(b"LessThan"); p = bpg.Prover(ctx, tr)
        p.defer_commitments(True)                                           # the three commitments of a statement in one launch
        _, vs = p.commit_many(values, blinds)
        right = bpg.LinearCombination.of(p.input(sc(bound))) if as_input else bpg.LinearCombination.of(sc(bound))
        bpg.LessThan(vs[0], values[0], right, sc(bound)).prove(p, [], [(values[1], vs[1]), (values[2], vs[2])])
        p.flush_commitments()
        return p, tr

    tmpl = assemble(*stmts[0], True)[0].template(ctx)
    items = [(b"".join(values), [], pre, b"".join(blinds), rng(k), 0, None, [sc(bound)]) for k, (bound, values, blinds) in enumerate(stmts)]
    split = {"assemble_and_commit": [], "prove_batch": []}

    def new_way():
        return tmpl.prove_batch_inputs(items, commit=True)

    def old_way():
        t1 = time.perf_counter()
        made = [assemble(bound, values, blinds, False) for bound, values, blinds in stmts]
        batch, coms = [], []
        for k, (p, tr) in enumerate(made):
            inst = p.instance()
            coms.append(b"".join(p.commitment(j) for j in range(3)))
            batch.append((inst, tr.state, inst.v_blinding, rng(k), 0))
        split["assemble_and_commit"].append(ms(t1))
        t2 = time.perf_counter()
        res = ctx.prove_batch(batch)
        split["prove_batch"].append(ms(t2))
        return [(proof, state, c) for (proof, state), c in zip(res, coms)]

    ways = {"template_inputs": new_way, "host_assembly": old_way}
    want = old_way()
    assert new_way() == want, "the template batch differs from the host assemblies with constants"
    split = {k: [] for k in split}
    T = {k: [] for k in ways}
    for r in range(a.reps):
        for name in (("template_inputs", "host_assembly") if r % 2 == 0 else ("host_assembly", "template_inputs")):
            t1 = time.perf_counter(); got = ways[name](); T[name].append(ms(t1))
            assert got == want, "repetition %d: %s differs" % (r, name)
    out = {"source_hash": bench.source_hash(), "gadget": "LessThan, public right-hand side", "n": tmpl.n, "N": 512, "items": K, "different_bounds": K, "reps": a.reps,
           "clock": "host clock around synchronised calls, ms", "ways_alternated": True, "commitments_inside_both": True,
           "proofs_states_commitments_equal": "warm-up and every repetition", "ms": {k: spread(v) for k, v in T.items()},
           "host_assembly_split_ms": {k: spread(v) for k, v in split.items()},
           "host_assembly_note": "assembled through the Python bindings (ctypes), one commitment launch per statement", "card_before": before}
    out["ms_median_ratio_host_over_template"] = round(out["ms"]["host_assembly"]["median"] / out["ms"]["template_inputs"]["median"], 2)
    ctx.profile_set(2)
    new_way()
    rep = ctx._report()
    ctx.profile_set(0)
    out["profile_template_inputs"] = {k: {"launches": rep.get(k, {}).get("count"), "ms": rep.get(k, {}).get("total_ms")}
                                      for k in ("k_input_slots", "k_witness_eval_batch", "k_bt_commit_v")}
    out["card_after"] = card_state()
    tmpl.free(); ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
