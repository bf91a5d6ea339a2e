#!/usr/bin/env python3
"""--count LessThan statements against as many DIFFERENT public bounds as ONE proof (1024: n = 388,096, N = 2^19), three ways.  Host clock around
synchronised calls; legs (a) and (b) alternate in one process, median of --reps.
  (a) one resident LessThan template with its bound as a public input, repeat_inputs(count) made ONCE; per proof assign(values, inputs=bounds) + prove.
  (b) the only way to that proof without public inputs through the repeat: ONE host assembly of the count-fold circuit with the bounds baked in as
      constants, instance(), upload(), prove.  The commitments are common to both legs, timed apart and in neither total.
  (c) count separate proofs by prove_batch_inputs(commit=False) on the single template: proving time and total proof bytes, and verify_batch of the count
      proofs against verify of the ONE proof of (a) after set_inputs(bounds) on a repeat that never held a witness.
Proofs (a) and (b) must be equal byte for byte in every repetition: the tool refuses to write its file otherwise.  Writes profiles/template_repeat_inputs.json
(--out) and prints the same JSON object."""
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
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_repeat_inputs.json"))
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    L, K = bpg.L, a.count
    sc = lambda x: (x % (1 << 256)).to_bytes(32, "little")
    rng = lambda k: hashlib.sha256(b"template-repeat-inputs %d" % k).digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    LC = bpg.LinearCombination.of
    ctx = bpg.Context(0)

    def statements(rep):
        """count (left, bound) pairs of repetition `rep`: bounds of every size up to 2^125, all different"""
        out = []
        for k in range(K):
            h = int.from_bytes(hashlib.sha256(b"bounds %d %d" % (rep, k)).digest(), "little")
            bound = 2 + (h >> 8) % (1 << (2 + h % 124))
            out.append(((h >> 140) % bound, bound))
        return out

    def blinds(rep, k):
        return [workloads.blinding("repeat-inputs-%d-%d" % (rep, k), i) for i in range(3)]

    split = {"commit": 0.0, "assemble": 0.0}                # seconds inside item(): the Pedersen commitments (commit, setup) and the gadget's rows (prove)

    def item(p, left, bound, bl, as_input):
        ls = sc(left)
        t0 = time.perf_counter()
        lcom, lvar = p.commit(ls, bl[0])
        g = bpg.LessThan(lvar, ls, LC(p.input(sc(bound))) if as_input else LC(sc(bound)), sc(bound))
        dcoms, derived = g.setup(p, [], bl[1:])
        t1 = time.perf_counter()
        g.prove(p, [], derived)
        split["commit"] += t1 - t0; split["assemble"] += time.perf_counter() - t1
        return [lcom] + dcoms

    def baked(rep, T):
        """leg (b): commit and assemble all statements in ONE prover, bounds as constants -> (instance, transcript state before the proof, commitments)"""
        t = bpg.Transcript(b"LessThan"); p = bpg.Prover(ctx, t)
        coms = []
        split["commit"] = split["assemble"] = 0.0
        for k, (left, bound) in enumerate(statements(rep)):
            coms += item(p, left, bound, blinds(rep, k), False)
        T["common_commit"].append(split["commit"] * 1e3); T["b_assemble"].append(split["assemble"] * 1e3)
        t0 = time.perf_counter(); inst = p.instance(); T["b_instance"].append(ms(t0))
        return inst, t.state, b"".join(coms)

    one = bpg.Prover(ctx, bpg.Transcript(b"LessThan"))
    item(one, 1, 2, blinds(-1, 0), True)
    tmpl = one.template(ctx)
    n1 = tmpl.n
    ctx.gens_ensure(1 << max(K * n1 - 1, 1).bit_length())
    t0 = time.perf_counter(); rep_c = tmpl.repeat_inputs(K); repeat_ms = ms(t0)
    names = ("common_commit", "b_assemble", "b_instance", "b_upload", "b_prove", "a_assign", "a_prove")
    T = {k: [] for k in names}
    proof_a = state_a = coms_a = bounds_a = None
    for r in range(a.reps + 1):                             # repetition 0 warms both legs and is dropped
        Tr = T if r else {k: [] for k in names}
        inst, state, coms = baked(r, Tr)
        bounds = b"".join(sc(b) for _, b in statements(r))
        t0 = time.perf_counter(); res = ctx.upload(inst); Tr["b_upload"].append(ms(t0))
        t0 = time.perf_counter(); want, after_b = res.prove(state, inst.v_blinding, rng(r)); Tr["b_prove"].append(ms(t0))
        res.free()
        t0 = time.perf_counter(); rep_c.assign(inst.v, inputs=bounds); Tr["a_assign"].append(ms(t0))
        t0 = time.perf_counter(); got, after_a = rep_c.prove(state, inst.v_blinding, rng(r)); Tr["a_prove"].append(ms(t0))
        if (got, after_a) != (want, after_b):
            sys.exit("repetition %d: the proof of the repeat with inputs differs from the proof of the host assembly with constants - nothing written" % r)
        proof_a, state_a, coms_a, bounds_a = got, state, coms, bounds
    med = {k: round(statistics.median(v), 3) for k, v in T.items()}
    out = {"count": K, "n": K * n1, "N": 1 << max(K * n1 - 1, 1).bit_length(), "reps": a.reps, "repeat_inputs_once_ms": round(repeat_ms, 3), "ms_median": med,
           "ms_all": {k: [round(x, 2) for x in v] for k, v in T.items()},
           "a_total_ms": round(med["a_assign"] + med["a_prove"], 3),
           "b_total_ms": round(med["b_assemble"] + med["b_instance"] + med["b_upload"] + med["b_prove"], 3),
           "note": "common_commit: the 3 x count Pedersen commitments, one Python call each, which both legs need for the transcript - in neither total",
           "proofs_equal": True, "one_proof_bytes": len(proof_a)}
    # (c) count separate proofs on the single template, and the verifier's side of both
    r = a.reps
    singles = []
    t0 = time.perf_counter()
    for k, (left, bound) in enumerate(statements(r)):
        t = bpg.Transcript(b"LessThan"); p = bpg.Prover(ctx, t)
        coms = item(p, left, bound, blinds(r, k), False)
        singles.append((p.instance(), t.state, bound, b"".join(coms)))
    c_assemble = ms(t0)
    items = [(inst.v, [], state, inst.v_blinding, rng(1000 + k), 0, None, [sc(bound)]) for k, (inst, state, bound, _) in enumerate(singles)]
    tmpl.prove_batch_inputs(items[:64])                     # warm
    t0 = time.perf_counter(); res = tmpl.prove_batch_inputs(items); c_prove = ms(t0)
    if any(x[0] is None for x in res):
        sys.exit("a separate proof failed - nothing written")
    shape = tmpl.repeat_inputs(K)                           # the verifier's circuit: it never holds a witness
    shape.set_inputs(bounds_a); shape.verify(state_a, coms_a, proof_a)     # warm
    t0 = time.perf_counter(); shape.set_inputs(bounds_a); set_ms = ms(t0)
    t0 = time.perf_counter(); st = shape.verify(state_a, coms_a, proof_a); one_ms = ms(t0)
    if st != 0:
        sys.exit("the one proof does not verify after set_inputs - nothing written")
    vitems = [(inst, state, coms, res[k][0]) for k, (inst, state, _, coms) in enumerate(singles)]
    ctx.verify_batch(vitems[:64])                           # warm
    t0 = time.perf_counter(); vres = ctx.verify_batch(vitems); batch_ms = ms(t0)
    if any(x != 0 for x in vres[0]):
        sys.exit("verify_batch rejected a separate proof - nothing written")
    verify = {"set_inputs_ms": round(set_ms, 3), "verify_one_proof_ms": round(one_ms, 3), "verify_batch_of_count_ms": round(batch_ms, 3)}
    out["separate_proofs"] = {"assemble_ms": round(c_assemble, 3), "prove_batch_inputs_ms": round(c_prove, 3), "total_proof_bytes": sum(len(x[0]) for x in res)}
    out["verify"] = verify
    shape.free(); rep_c.free(); tmpl.free(); ctx.close()
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
