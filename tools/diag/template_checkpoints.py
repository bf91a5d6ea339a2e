#!/usr/bin/env python3
"""What a fresh witness costs on the hash-chain circuits, three ways, on one box: ResidentCircuit.assign WITH checkpoints (the preparation of their values
included: the host sponge's states, or the read-back from the resident tree), assign WITHOUT, and host assembly + flatten + upload.  Circuits: the cfg 3
preimage (--preimage-bytes 2130: 67 absorbed blocks), a Merkle path (--path-depth 20) at one index of a resident tree, and the full tree of --tree-leaves 512
committed leaves with its checkpoints taken from MerkleTree.nodes.  The commitments are common to the three ways and are not timed.  Host clock around
synchronised calls; the ways alternate in every repetition (the order rotates); median and min..max of --reps after a warm-up in which the three ways'
PROOFS are compared byte for byte.  Beside the times: the schedule levels, every level's launch time and the verify launch from the engine's event profile
(a pass of its own), and what a read-only query says about other work on the card.  Writes one JSON object (profiles/template_checkpoints.json)."""
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

WAYS = ("assign_checkpointed", "assign_plain", "host_assembly")
SEED = hashlib.sha256(b"template checkpoints tool").digest()
ms = lambda t0: (time.perf_counter() - t0) * 1e3


def card_summary(raw):
    """of rocm-smi's answer: the busy and memory percentages of every card and how many processes have a card open"""
    cards = {k: {"use_pct": v.get("GPU use (%)"), "vram_pct": v.get("GPU Memory Allocated (VRAM%)")} for k, v in raw.items() if k.startswith("card")}
    return {"cards": cards, "processes_with_a_card_open": len(raw.get("system", {}))}


def card_state():
    """what else is on the card, as far as a read-only query tells"""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse", "--showpids", "--json"], capture_output=True, text=True, timeout=20)
        return card_summary(json.loads(r.stdout)) if r.returncode == 0 else {"unknown": r.stderr[-200:]}
    except Exception as e:        # no tool, no answer: say so
        return {"unknown": repr(e)}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


class Case:
    """one circuit: fresh(k) -> a witness (whatever the three ways need, commitments made); the ways are methods that time themselves"""

    def __init__(self, bpg, ctx):
        self.bpg, self.ctx = bpg, ctx

    def start(self):
        """templates from witness 0: one with checkpoints, one without"""
        w = self.fresh(0)
        self.host_assembly(w, {}).free()
        p = w["prover"]
        rows = [p.num_constraints() - 1]
        self.ctx.gens_ensure(1 << max(p.get_num_multiplications() - 1, 1).bit_length())
        self.ck_vars = self.checkpoint_vars(p)
        self.tmpl_ck = p.template(self.ctx, param_rows=rows, checkpoints=self.ck_vars)
        self.tmpl_plain = p.template(self.ctx, param_rows=rows)
        self.n = p.get_num_multiplications()

    def host_assembly(self, w, T):
        """assemble, flatten, upload -> the resident circuit (the caller frees it)"""
        t0 = time.perf_counter(); w["assemble"](); a = ms(t0)
        t1 = time.perf_counter(); inst = w["prover"].instance(); b = ms(t1)
        t2 = time.perf_counter(); res = self.ctx.upload(inst); c = ms(t2)
        T.setdefault("host_assembly", []).append(ms(t0))
        for k, x in (("host_assemble", a), ("host_flatten", b), ("host_upload", c)):
            T.setdefault(k, []).append(x)
        w["inst"] = inst
        return res

    def assign_checkpointed(self, w, T):
        t0 = time.perf_counter(); values = self.checkpoint_values(w); a = ms(t0)
        self.tmpl_ck.assign(w["v"], [w["param"]], checkpoints=values)
        T.setdefault("assign_checkpointed", []).append(ms(t0)); T.setdefault("checkpoint_preparation", []).append(a)

    def assign_plain(self, w, T):
        t0 = time.perf_counter(); self.tmpl_plain.assign(w["v"], [w["param"]]); T.setdefault("assign_plain", []).append(ms(t0))

    def run(self, reps):
        self.start()
        # warm-up: the three ways give the same proof bytes
        w = self.fresh(1)
        res = self.host_assembly(w, {}); state, vb = w["transcript"].state, w["inst"].v_blinding
        want = res.prove(state, vb, SEED)[0]; res.free()
        self.assign_checkpointed(w, {}); got_ck = self.tmpl_ck.prove(state, vb, SEED)[0]
        self.assign_plain(w, {}); got_plain = self.tmpl_plain.prove(state, vb, SEED)[0]
        assert got_ck == want and got_plain == want, "the three ways give different proofs"
        T = {}
        for k in range(reps):
            w = self.fresh(2 + k)
            for j in range(3):
                way = WAYS[(k + j) % 3]
                if way == "host_assembly":
                    self.host_assembly(w, T).free()
                else:
                    getattr(self, way)(w, T)
        # the device's share, from the event profile, in a pass of its own
        out = {"n": self.n, "checkpoints": len(self.ck_vars), "reps": reps, "proofs_equal_in_warm_up": True, "ms": {k: spread(v) for k, v in T.items()}}
        for name, fn in (("checkpointed", self.assign_checkpointed), ("plain", self.assign_plain)):
            self.ctx.profile_set(2)
            fn(w, {})
            rep = self.ctx._report()
            self.ctx.profile_set(0)
            out["profile_" + name] = {"levels": rep.get("k_witness_eval", {}).get("count"), "level_ms": rep.get("_witness_launch_ms"),
                                      "k_witness_eval_ms": rep.get("k_witness_eval", {}).get("total_ms"),
                                      "k_witness_ck_verify_ms": rep.get("k_witness_ck_verify", {}).get("total_ms")}
        self.tmpl_ck.free(); self.tmpl_plain.free()
        self.finish()
        return out

    def finish(self):
        pass


class Preimage(Case):
    def __init__(self, bpg, ctx, nbytes):
        super().__init__(bpg, ctx); self.nbytes = nbytes

    def fresh(self, k):
        bpg = self.bpg
        from bulletproofs_gadgets_amd import workloads
        cfg = "ck-pre-%d" % k
        pre = workloads.synth(cfg, 0, self.nbytes)
        image = bpg.mimc_hash(pre)
        t = bpg.Transcript(b"MiMCHash"); p = bpg.Prover(self.ctx, t)
        g = bpg.MimcHash256(image)
        nblocks = (self.nbytes + 31) // 32
        scalars, _, wvars = bpg.commit(p, pre, [workloads.blinding(cfg, i) for i in range(nblocks)])
        _, derived = g.setup(p, scalars, [workloads.blinding(cfg, 1000), workloads.blinding(cfg, 1001)])
        v = b"".join(scalars) + b"".join(s for s, _ in derived)
        blocks = list(scalars[:-1]) + [derived[0][0]] if len(derived) == 2 else list(scalars) + [derived[0][0]]
        return {"prover": p, "transcript": t, "assemble": lambda: g.prove(p, wvars, derived), "v": v, "blocks": blocks,
                "param": bpg.scalar_op("sub", bytes(32), image)}

    def checkpoint_vars(self, p):
        return [var for var, _, _ in p.noted()]

    def checkpoint_values(self, w):
        return self.bpg.mimc_sponge_states(w["blocks"])


class Path(Case):
    """one index of a resident tree of 2^depth leaves; a fresh witness = the leaf replaced (MerkleTree.update) and the tree's new siblings"""

    def __init__(self, bpg, ctx, depth):
        super().__init__(bpg, ctx)
        self.depth, self.index = depth, (0x5a5a5 % (1 << depth))
        raw = hashlib.shake_256(b"ck path leaves").digest(32 << depth)
        leaves = b"".join(raw[i:i + 31] + bytes([raw[i + 31] & 0x0f]) for i in range(0, 32 << depth, 32))     # below 2^252 < l: canonical
        t0 = time.perf_counter(); self.tree = ctx.merkle_tree(leaves); self.tree_build_ms = ms(t0)
        from bulletproofs_gadgets_amd import workloads
        self.pattern, self.order = workloads.merkle_path_pattern(self.index, depth)

    def fresh(self, k):
        bpg = self.bpg
        from bulletproofs_gadgets_amd import workloads
        cfg = "ck-path-%d" % k
        leaf = workloads.synth(cfg, 0, 31) + b"\x07"
        self.tree.update([self.index], [leaf])
        sib, root = self.tree.paths([self.index])[0], self.tree.root()
        values = [leaf if what == "leaf" else sib[j] for what, j in self.order]
        t = bpg.Transcript(b"MerklePath"); p = bpg.Prover(self.ctx, t)
        _, vs = p.commit_many(values, [workloads.blinding(cfg, i) for i in range(len(values))])
        g = bpg.MerkleTree256(root, [], bpg.vars_to_lc(vs), self.pattern)
        return {"prover": p, "transcript": t, "assemble": lambda: g.prove(p, [], []), "v": b"".join(values), "param": bpg.scalar_op("sub", bytes(32), root)}

    def checkpoint_vars(self, p):
        return [var for var, _, last in p.noted() if last]

    def checkpoint_values(self, w):
        return self.tree.path_nodes([self.index])[0]

    def finish(self):
        self.tree.free()


class Tree(Case):
    """the full tree, every leaf committed; a fresh witness = fresh leaves and a resident tree built over them (the build is timed apart: a tree server has it)"""

    def __init__(self, bpg, ctx, leaves):
        super().__init__(bpg, ctx)
        self.leaves, self.depth = leaves, leaves.bit_length() - 1
        self.build_ms, self.trees = [], []
        # the node digests in assembly order (children before their parent, left before right) as (level, index), level 0 = the root
        def post(level, i):
            return (post(level + 1, 2 * i) + post(level + 1, 2 * i + 1) if level + 1 < self.depth else []) + [(level, i)]
        self.node_order = post(0, 0)

    def fresh(self, k):
        bpg = self.bpg
        from bulletproofs_gadgets_amd import workloads
        cfg = "ck-tree-%d" % k
        leaf_be = [b"\x07" + workloads.synth(cfg, i, 31) for i in range(self.leaves)]
        scal = [bpg.be_to_scalar(b) for b in leaf_be]
        t0 = time.perf_counter(); tree = self.ctx.merkle_tree(scal); self.build_ms.append(ms(t0))
        self.trees.append(tree)
        root = tree.root()
        t = bpg.Transcript(b"MerkleTree"); p = bpg.Prover(self.ctx, t)
        _, _, wvars = bpg.commit_all_single(p, leaf_be, [workloads.blinding(cfg, i) for i in range(self.leaves)])
        g = bpg.MerkleTree256(root, [], bpg.vars_to_lc(wvars), workloads.full_tree_pattern(self.leaves))
        return {"prover": p, "transcript": t, "assemble": lambda: g.prove(p, [], []), "v": b"".join(scal), "param": bpg.scalar_op("sub", bytes(32), root), "tree": tree}

    def checkpoint_vars(self, p):
        return [var for var, _, last in p.noted() if last]

    def checkpoint_values(self, w):
        levels = [w["tree"].nodes(level) for level in range(self.depth)]
        return [levels[level][i] for level, i in self.node_order]

    def finish(self):
        for t in self.trees:
            t.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preimage-bytes", type=int, default=2130)
    ap.add_argument("--path-depth", type=int, default=20)
    ap.add_argument("--tree-leaves", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_checkpoints.json"))
    a = ap.parse_args()
    before = card_state()
    import bulletproofs_gadgets_amd as bpg
    ctx = bpg.Context(0)
    out = {"reps": a.reps, "ways_alternated": True, "clock": "host clock around synchronised calls, ms", "card_before": before}
    out["preimage"] = dict(Preimage(bpg, ctx, a.preimage_bytes).run(a.reps), preimage_bytes=a.preimage_bytes)
    path = Path(bpg, ctx, a.path_depth)
    out["path"] = dict(path.run(a.reps), depth=a.path_depth, index=path.index, tree_build_ms=round(path.tree_build_ms, 3))
    tree = Tree(bpg, ctx, a.tree_leaves)
    out["tree"] = dict(tree.run(a.reps), leaves=a.tree_leaves, tree_build_ms=spread(tree.build_ms))
    out["shared_variants_last"] = ctx.schedule().get("shared_variants_last")
    out["card_after"] = card_state()
    ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
