#!/usr/bin/env python3
"""What a fresh witness costs: host assembly + upload (the only way before circuit templates) against ResidentCircuit.assign, on the full MiMC Merkle
tree of --leaves committed leaves (512: n = 993,384, N = 2^20).  Host clock around synchronised calls, the two ways alternated in every repetition,
median of --reps; every proof of the template is compared with the host-assembled one.  Parts timed for the host way: the gadget's prove() call (the
assembly), instance() (flatten), upload(); common to both ways and timed apart: the leaf commitments.  Then a sequence of fresh witnesses on one context
with the blinding chain drawn one proof ahead: proofs per second with assembly + upload per proof against assign per proof.  k_witness_eval's launches,
device time and the time of every launch (= level) come from the engine's event profile in a pass of its own; `mix` is assign beside --mix-streams
proving streams, `cfg3_preimage` the 67-level MiMC preimage.  Prints one JSON object (profiles/template_assign.json)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def cfg3(bpg, workloads, ctx, reps):
    """the 2^16 MiMC preimage (67 absorbed blocks: 67 levels of ONE segment): host assembly + upload against assign"""
    T = {"assemble_commit": [], "instance": [], "upload": [], "assign": []}
    base = workloads.mimc_preimage(ctx, seed=1)
    tmpl = base.prover.template(ctx, param_rows=[base.prover.num_constraints() - 1])
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    for k in range(2, 2 + reps):
        t0 = time.perf_counter(); x = workloads.mimc_preimage(ctx, seed=k); T["assemble_commit"].append(ms(t0))
        t0 = time.perf_counter(); inst = x.prover.instance(); T["instance"].append(ms(t0))
        t0 = time.perf_counter(); res = ctx.upload(inst); T["upload"].append(ms(t0)); res.free()
        image = bpg.mimc_hash(workloads.synth("cfg3-%d" % k, 0, 2130))
        minus = ((bpg.L - int.from_bytes(image, "little")) % bpg.L).to_bytes(32, "little")
        t0 = time.perf_counter(); tmpl.assign(inst.v, [minus]); T["assign"].append(ms(t0))
    tmpl.free()
    return {"n": inst.n, "levels": 67, "ms_median": {k: round(statistics.median(v), 3) for k, v in T.items()}}


def mix(bpg, a, tmpl, ws, inst, state, rng):
    """--mix-streams proving streams (a context, a thread and a chain worker each) prove one resident 2^20 witness over and over, the chain of the next
    proof started before the current one is proved; windows of --mix-seconds alternate between the streams alone and the streams beside a seventh thread
    that assigns fresh witnesses to the template without pause.  Reported: sustained ms per proof of the streams in each window, and assign's wall time
    inside the mix."""
    import threading
    L = bpg.L
    ctxs = [bpg.Context(0) for _ in range(a.mix_streams)]
    circ = []
    for c in ctxs:
        c.gens_ensure(1 << max(inst.n - 1, 1).bit_length()); circ.append(c.upload(inst))
    stop, done, lock = threading.Event(), [0], threading.Lock()

    def stream(i):
        c, r = ctxs[i], circ[i]
        k = 0
        c.blinding_begin(state, inst.v_blinding, rng(1000 * i), 1 << 20)
        while not stop.is_set():
            c.blinding_begin(state, inst.v_blinding, rng(1000 * i + k + 1), 1 << 20)
            r.prove(state, inst.v_blinding, rng(1000 * i + k)); k += 1
            with lock:
                done[0] += 1

    assigning, assign_ms = threading.Event(), []
    vals = []
    for leaf_be, blind, root in ws[:4]:
        vals.append((b"".join(bpg.be_to_scalar(b) for b in leaf_be), ((L - int.from_bytes(root, "little")) % L).to_bytes(32, "little")))

    def assigner():
        k = 0
        while not stop.is_set():
            if not assigning.is_set():
                time.sleep(0.005); continue
            v, mr = vals[k % len(vals)]; k += 1
            t0 = time.perf_counter(); tmpl.assign(v, [mr]); assign_ms.append((time.perf_counter() - t0) * 1e3)

    th = [threading.Thread(target=stream, args=(i,)) for i in range(a.mix_streams)] + [threading.Thread(target=assigner)]
    for t in th:
        t.start()
    time.sleep(2.0)                                                     # every stream past its first proofs
    windows = []
    for w in range(4):
        (assigning.set if w % 2 else assigning.clear)()
        time.sleep(0.3)
        with lock:
            n0 = done[0]
        t0 = time.perf_counter(); time.sleep(a.mix_seconds)
        with lock:
            n1 = done[0]
        windows.append({"assign_running": bool(w % 2), "proofs": n1 - n0, "ms_per_proof": round((time.perf_counter() - t0) * 1e3 / max(n1 - n0, 1), 2)})
    stop.set()
    for t in th:
        t.join()
    for c, r in zip(ctxs, circ):
        r.free(); c.close()
    return {"streams": a.mix_streams, "windows": windows, "assigns": len(assign_ms),
            "assign_ms_median_in_mix": round(statistics.median(assign_ms), 2) if assign_ms else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sequence", type=int, default=6)
    ap.add_argument("--mix-streams", type=int, default=6, help="proving streams of the mix leg (0: skip it)")
    ap.add_argument("--mix-seconds", type=float, default=5.0)
    a = ap.parse_args()
    import bulletproofs_gadgets_amd as bpg
    from bulletproofs_gadgets_amd import workloads
    L = bpg.L
    ctx = bpg.Context(0)
    pattern = workloads.full_tree_pattern(a.leaves)
    rng = lambda k: hashlib.sha256(b"template-assign %d" % k).digest()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3

    def leaves_of(seed):
        cfg = "tmpl-%d" % seed
        leaf_be = [b"\x07" + workloads.synth(cfg, i, 31) for i in range(a.leaves)]
        probe = bpg.Prover(None, bpg.Transcript(b"probe"))                 # the root is an input of a real prover; this stands in for knowing it
        bpg.MerkleTree256(bytes(32), [bpg.be_to_scalar(b) for b in leaf_be], [], pattern.replace("W", "I")).prove(probe, [], [])
        return leaf_be, [workloads.blinding(cfg, i) for i in range(a.leaves)], probe.instance().aO[-32:]

    def host_way(w, T):
        """commit, assemble, flatten, upload: returns (resident circuit, instance, transcript state)"""
        leaf_be, blind, root = w
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        t0 = time.perf_counter(); _, _, wvars = bpg.commit_all_single(p, leaf_be, blind); T["commit"].append(ms(t0))
        t0 = time.perf_counter(); bpg.MerkleTree256(root, [], bpg.vars_to_lc(wvars), pattern).prove(p, [], []); T["assemble"].append(ms(t0))
        t0 = time.perf_counter(); inst = p.instance(); T["instance"].append(ms(t0))
        t0 = time.perf_counter(); res = ctx.upload(inst); T["upload"].append(ms(t0))
        return res, inst, t.state, p

    def template_way(tmpl, w, T):
        """commit (for the transcript), assign: returns (values, blindings, transcript state)"""
        leaf_be, blind, root = w
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        t0 = time.perf_counter(); bpg.commit_all_single(p, leaf_be, blind); T["commit_t"].append(ms(t0))
        v = b"".join(bpg.be_to_scalar(b) for b in leaf_be)
        minus_root = ((L - int.from_bytes(root, "little")) % L).to_bytes(32, "little")
        t0 = time.perf_counter(); tmpl.assign(v, [minus_root]); T["assign"].append(ms(t0))
        return b"".join(blind), t.state

    ws = [leaves_of(s) for s in range(a.reps + a.sequence + 2)]
    T = {k: [] for k in ("commit", "assemble", "instance", "upload", "commit_t", "assign", "prove_host", "prove_template")}
    res, inst, state, p0 = host_way(ws[0], {k: [] for k in T})
    state0 = state
    ctx.gens_ensure(1 << max(inst.n - 1, 1).bit_length())
    tmpl = p0.template(ctx, param_rows=[p0.num_constraints() - 1])
    res.prove(state, inst.v_blinding, rng(0)); res.free()                                       # warm
    for k in range(1, a.reps + 1):
        res, inst, state, _ = host_way(ws[k], T)
        t0 = time.perf_counter(); want, _ = res.prove(state, inst.v_blinding, rng(k)); T["prove_host"].append(ms(t0)); res.free()
        vb, state2 = template_way(tmpl, ws[k], T)
        t0 = time.perf_counter(); got, _ = tmpl.prove(state2, vb, rng(k)); T["prove_template"].append(ms(t0))
        assert state2 == state and got == want, "the template's proof differs from the host assembly's"
    out = {"leaves": a.leaves, "n": inst.n, "reps": a.reps, "ms_median": {k: round(statistics.median(v), 3) for k, v in T.items()},
           "ms_all": {k: [round(x, 2) for x in v] for k, v in T.items()}}
    # device time of the evaluation alone (event profile, a pass of its own)
    ctx.profile_set(2)
    template_way(tmpl, ws[1], {k: [] for k in T})
    rep = ctx._report()
    ctx.profile_set(0)
    k = rep.get("k_witness_eval", {})
    out["k_witness_eval"] = {"launches": k.get("count"), "device_ms": k.get("total_ms"), "level_ms": rep.get("_witness_launch_ms"),
                             "level_segments": [a.leaves >> (1 + l // 2) for l in range(len(rep.get("_witness_launch_ms", [])))]}
    if a.mix_streams:
        out["mix"] = mix(bpg, a, tmpl, ws, p0.instance(), state0, rng)
    if a.leaves >= 64:
        out["cfg3_preimage"] = cfg3(bpg, workloads, ctx, a.reps)
    # a sequence of fresh witnesses, the chain of proof k+1 started before proof k is proved
    seq = ws[a.reps + 1:a.reps + 1 + a.sequence]
    dummy = {k: [] for k in T}

    def sequence(prepare):
        nxt = prepare(seq[0], 0)
        ctx.blinding_begin(nxt[1], nxt[2], rng(100), 1 << 20)
        t0 = time.perf_counter(); proofs = []
        for k in range(len(seq)):
            cur = nxt
            if k + 1 < len(seq):
                nxt = prepare(seq[k + 1], k + 1)      # the host way assembles and uploads witness k+1 here, on the proving thread, under chain k
            proofs.append(cur[3]())
            if k + 1 < len(seq):
                ctx.blinding_begin(nxt[1], nxt[2], rng(100 + k + 1), 1 << 20)
        return len(seq) / (time.perf_counter() - t0), proofs

    def prep_host(w, k):
        res, inst, state, _ = host_way(w, dummy)
        def go():
            pr = res.prove(state, inst.v_blinding, rng(100 + k))[0]; res.free(); return pr
        return res, state, inst.v_blinding, go

    def prep_template(w, k):
        # the template holds ONE witness: assign when the proof is made, only the commitments are prepared ahead
        leaf_be, blind, root = w
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(ctx, t)
        bpg.commit_all_single(p, leaf_be, blind)
        v = b"".join(bpg.be_to_scalar(b) for b in leaf_be)
        minus_root = ((L - int.from_bytes(root, "little")) % L).to_bytes(32, "little")
        state, vb = t.state, b"".join(blind)
        def go():
            tmpl.assign(v, [minus_root]); return tmpl.prove(state, vb, rng(100 + k))[0]
        return tmpl, state, vb, go

    r_host, p_host = sequence(prep_host)
    r_tmpl, p_tmpl = sequence(prep_template)
    assert p_host == p_tmpl
    out["sequence"] = {"proofs": len(seq), "proofs_per_s_host_assembly": round(r_host, 3), "proofs_per_s_assign": round(r_tmpl, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
