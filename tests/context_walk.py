"""A model-based sequence test of ONE context: a catalogue of small operations over every family of entry points, the exact result of each computed on
the CPU independently of order, and walks that run them on one context in orders that make every family follow every family.

What a context keeps from call to call - one arena for the large buffers of every entry point, the caches of window tables, merge sets and row views, the
generator tables that grow under resident circuits, the sticky flags and the blinding slab ("What a context keeps between calls") - is
correct only while the lifetimes never overlap in stream order.  A test of one feature on a fresh context cannot see a neighbour's leftovers; a walk can.

    Op            family, variant, prepare() -> Expect (cached for the process, never touches a context), run(env) -> result, same(want, got)
    CATALOGUE     family -> its variants, in rotation order
    build_walk    an Eulerian circuit of the complete directed graph on the families, loops included: all 17 x 17 ordered pairs are adjacent, 290 steps
    PINNED        short hand-written orders for the interactions the engine's code suggests, each with its reason; PINNED_TWO: such orders for two contexts
    run_walk      one context (or two of one device, dealt the steps alternately), the resident set uploaded once, a comparison after every step
    replay        run_walk on a list of "family/variant" names - what a WalkMismatch prints

Expectations come from the references the suite already trusts and from nothing else: the CPU oracle (oracle_lib: prove, verify, msm, pedersen_commit,
mimc_sponge, the generator chain), the device-less host assembly with the oracle's commitments (HostProver) and the device-less mirror of the R1CS check
(bpg.test_check_host).  No expectation is taken from a GPU call.

Sizes are the smallest that take a distinct memory path and stay at N <= 1024: a 40-bit range proof (N = 64), the 64-bit BoundsCheck (n = N = 128), the
one-block MiMC preimage (n = 972, N = 1024: 52 padding generators, the size that takes the bucket-method path once BPG_TT_LG / BPG_TT_ORIG_LG say so), the
8-bit BoundsCheck (n = 16) and SetMembership (n = 6) for repeats and joins, the 36-multiplier checkpoint chain, LessThan against a public bound (N = 512), the
hand-made gate circuit (n = 10, N = 16), three Inequality statements against three public values (n = 9), a depth-11 tree grown to 606 leaves in both layouts,
a depth-11 keyed tree of 122 keys (7, then 100 more past the minimum capacity of 64, then 25 of which 15 are new)."""
import contextlib
import copy
import ctypes as C
import functools
import gc
import hashlib
import random

import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
import checkpoint_cases as CK
import gate_cases as GC
import keyed_cases as KC
import repeat_inputs_cases as RC
import template_inputs_cases as TC
from test_template_repeat_host import CIRCUITS, SET_INSTANCE, bounds8_item, constant_term

L = bpg.L
sc = lambda x: (x % L).to_bytes(32, "little")
START_CAPACITY = 1024
MAX_GROWS = 3                                   # 1024 -> 2048 -> 4096 -> 8192
ERR_INVALID, ERR_DEVICE, ERR_MISMATCH = 4, 7, 9
BAD8 = [sc(7), sc((1 << 8) + 5), sc(255 - ((1 << 8) + 5))]      # a + b = max - min holds, the 8-bit range proof of a does not


def rng(tag):
    return hashlib.sha256(("context walk %s" % tag).encode()).digest()


def rs(tag, i):
    return sc(int.from_bytes(hashlib.sha512(("context walk %s %d" % (tag, i)).encode()).digest(), "little"))


# ------------------------------------------------------------------------------------------------ host assembly without a device
class HostProver(bpg.Prover):
    """Assembly-only product prover (no device context); Pedersen commitments by the oracle, registered with commit_precomputed."""
    def __init__(self, ctx, transcript):
        super().__init__(None, transcript)

    def commit(self, v, v_blinding):
        com = O.pedersen_commit(sc(int.from_bytes(v, "little")), v_blinding)
        return com, self.commit_precomputed(v, v_blinding, com)

    def commit_many(self, vs, blindings):
        out = [self.commit(v, b) for v, b in zip(vs, blindings)]
        return [c for c, _ in out], [x for _, x in out]

    def gadget_setup(self, g, witnesses, blindings):
        """Gadget::setup = preprocess + one commit per derived scalar (reference src/gadget.rs:18-38)"""
        derived = g.preprocess(witnesses)
        coms, out = [], []
        for s, b in zip(derived, blindings):
            com, v = self.commit(s, b)
            coms.append(com); out.append((s, v))
        return coms, out


@contextlib.contextmanager
def host_assembly():
    """while open, Gadget.setup on a HostProver commits through it (the case builders of the neighbouring tests call g.setup(prover, ...) directly)"""
    old = bpg.Gadget.setup

    def setup(self, prover, witnesses, blindings):
        if isinstance(prover, HostProver):
            return prover.gadget_setup(self, witnesses, blindings)
        return old(self, prover, witnesses, blindings)
    bpg.Gadget.setup = setup
    try:
        yield
    finally:
        bpg.Gadget.setup = old


def to_oracle(inst):
    return O.FlatCircuit(inst.n, inst.m, inst.aL or None, inst.aR or None, inst.aO or None, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)


@functools.lru_cache(maxsize=None)
def ogens(capacity):
    return O.Gens(capacity)


@functools.lru_cache(maxsize=None)
def state_before(label):
    """the transcript as Prover::new leaves it, before any "V" append"""
    t = bpg.Transcript(label)
    bpg.Prover(None, t)
    return t.state


class HostCase:
    """one host assembly: instance with witness, transcript after the commitments, the oracle's commitments, and the verifier's side where a replay is known"""
    def __init__(self, prover, transcript, commitments, label, replay=None):
        self.prover, self.inst, self.state, self.label = prover, prover.instance(), transcript.state, label
        self.coms = b"".join(commitments)
        self.N = 1
        while self.N < self.inst.n:
            self.N *= 2
        self.vinst, self.vstate, self._proofs = None, self.state, {}
        if replay is not None:
            v = bpg.Verifier(bpg.Transcript(label))
            replay(v)
            self.vinst, self.vstate = v.instance(), v.transcript.state
            assert self.vstate == self.state and self.vinst.commitments == self.coms

    def prove(self, seed, flags=0):
        """the oracle's (proof, transcript state after)"""
        if (seed, flags) not in self._proofs:
            rc, proof, after = O.prove(ogens(self.N), self.state, to_oracle(self.inst), self.inst.v_blinding, seed, flags | O.FLAG_FAST_MSM)
            assert rc == 0
            self._proofs[seed, flags] = (proof, after)
        return self._proofs[seed, flags]

    def verify(self, proof):
        """the oracle verifier's status on the verifier-side circuit (the prover-side rows where no replay is known: the same rows)"""
        return O.verify(ogens(self.N), self.vstate, to_oracle(self.vinst or self.inst), self.coms, proof)

    def claim(self, proof, status=0):
        return (self, proof, status)


def _assembled(a, label):
    return HostCase(a.prover, a.transcript, a.commitments, label, a.replay)


@functools.lru_cache(maxsize=None)
def b64(seed):
    """the 64-bit BoundsCheck: n = N = 128, m = 3"""
    with host_assembly():
        return _assembled(workloads.bounds_check_64(None, seed=seed, prover_cls=HostProver), b"BoundsCheck")


@functools.lru_cache(maxsize=None)
def mimc(seed):
    """the one-block MiMC preimage: n = 972, N = 1024"""
    with host_assembly():
        c = _assembled(workloads.mimc_preimage(None, nbytes=20, seed=seed, prover_cls=HostProver), b"MiMCHash")
    assert (c.inst.n, c.N) == (972, 1024)
    return c


@functools.lru_cache(maxsize=None)
def rp40():
    """a 40-bit range proof of a constant: 40 multipliers, N = 64 (24 padding generators), no commitments"""
    t = bpg.Transcript(b"RangeProof")
    p = HostProver(None, t)
    x = bpg.be_to_scalar(bytes([1, 2, 3, 4, 1]))
    bpg.range_proof(p, x, 40, x)
    return HostCase(p, t, [], b"RangeProof", lambda v: bpg.range_proof(v, x, 40))


@functools.lru_cache(maxsize=None)
def mixed(parts, tag, bad=None):
    """ONE prover that assembles the gadget code of `parts` = ((name, count), ...) part by part, item by item - the circuit a repeat or a join makes on the
    device; bad = (part, item): that bounds8 item holds an out-of-range value.  .params: the constant terms of the parameter rows, in order"""
    label = CIRCUITS[parts[0][0]][1] if len(parts) == 1 else b"MixedStatement"
    t = bpg.Transcript(label)
    p = HostProver(None, t)
    rows = []
    with host_assembly():
        for k, (name, count) in enumerate(parts):
            for i in range(count):
                if bad == (k, i):
                    rows += bounds8_item(p, "%s-part%d" % (tag, k), i, BAD8)
                else:
                    rows += CIRCUITS[name][0](p, "%s-part%d" % (tag, k), i)
    coms = [p.commitment(i) for i in range(p.num_committed())]

    def replay(v):
        """the verifier's assembly of the same statement: per item its commitments, then the gadget"""
        at = 0
        for name, count in parts:
            for _ in range(count):
                if name == "bounds8":
                    vs = bpg.verifier_commit(v, coms[at:at + 3]); at += 3
                    bpg.BoundsCheck(b"\x00", b"\xff").verify(v, vs[:1], vs[1:])
                else:
                    vs = bpg.verifier_commit(v, coms[at:at + 6]); at += 6
                    bpg.SetMembership(vs[0], None, SET_INSTANCE, None).verify(v, vs[1:3], vs[3:])
    c = HostCase(p, t, coms, label, replay if all(name in ("bounds8", "set3") for name, _ in parts) else None)
    c.params = [constant_term(c.inst, r) for r in rows]
    c.param_rows = rows
    return c


def b8(tag, K=1, bad_item=None):
    return mixed((("bounds8", K),), tag, None if bad_item is None else (0, bad_item))


@functools.lru_cache(maxsize=None)
def chain(seed):
    a = CK.chain(None, seed=seed, prover_cls=HostProver)
    c = HostCase(a.prover, a.transcript, a.commitments, b"CheckpointChain")
    c.ck_vars, c.ck_values = a.ck_vars, list(a.ck_values)
    c.param_rows = [CK.last_row(a)]
    c.params = [CK.constant_term(c.inst, c.param_rows[0])]
    return c


@functools.lru_cache(maxsize=None)
def less_than(left, bound, as_inputs, tag):
    with host_assembly():
        a = TC.less_than(None, left, bound, as_inputs, tag=tag, prover_cls=HostProver)
    c = HostCase(a.prover, a.transcript, a.commitments, b"LessThan", None if as_inputs else a.replay)
    c.inputs = a.inputs
    return c


@functools.lru_cache(maxsize=None)
def hand(inputs, values, tag="hand10"):
    """the UNGATED yardstick of the hand-made gate circuit: gate_cases.hand10 with the public values baked in as constants, coefficient by coefficient - an
    assembly that knows nothing of inputs or gates.  n = 10, N = 16, m = 2, 13 rows"""
    a = GC.hand10(inputs, values, False, prover_cls=HostProver, tag=tag)
    c = HostCase(a.prover, a.transcript, a.commitments, b"hand10")
    assert (c.inst.n, c.N, c.inst.m) == (GC.HAND_N, 16, 2)
    return c


def hand_vector(k):
    return hand(GC.HAND_INPUTS[k], GC.HAND_VALUES[k])


def hand_inputs(k):
    return [sc(x) for x in GC.HAND_INPUTS[k]]


@functools.lru_cache(maxsize=None)
def hand_template():
    """the GATED assembly of vector 0: the public values are inputs, the products input * variable are gates"""
    return GC.hand10(GC.HAND_INPUTS[0], GC.HAND_VALUES[0], True, prover_cls=HostProver)


REPEAT_INPUTS_PARTS = (("inequality", tuple(RC.ARGS["inequality"][:3])),)      # the smallest repeat of repeat_inputs_cases: K = 3, n = 9, N = 16, m = 12


@functools.lru_cache(maxsize=None)
def inequality3():
    """ONE host assembly of three Inequality statements with their three public right-hand sides baked in as constants, and the verifier's replay of it"""
    parts = [(name, list(args)) for name, args in REPEAT_INPUTS_PARTS]
    with host_assembly():
        a = RC.Assembly(parts, False, prover_cls=HostProver, tag="walk-repeat")
    c = HostCase(a.prover, a.transcript, a.commitments, b"Inequality")
    v = RC.replay(parts, a.commitments)
    c.vinst, c.vstate = v.instance(), v.transcript.state
    assert c.vstate == c.state and c.vinst.commitments == c.coms and (c.inst.n, c.N) == (9, 16)
    c.inputs, c.params = list(a.inputs), list(a.params)
    return c


@functools.lru_cache(maxsize=None)
def inequality_template():
    """the gadget code assembled once with the right-hand side as an input, from an item no statement of the walk uses"""
    with host_assembly():
        return RC.template_of("inequality", prover_cls=HostProver)


class Crossed:
    """the statement of `rows` claimed for the commitments of `held` (the transcript before a proof holds the label and the commitments, nothing of the
    rows): what a verifier who is handed other constants than the prover's judges.  Stands where a HostCase stands in a claim."""
    def __init__(self, rows, held):
        assert rows.inst.m == held.inst.m and rows.N == held.N and rows.label == held.label
        self.inst, self.vinst, self.N, self.label = rows.inst, rows.vinst, rows.N, rows.label
        self.state, self.vstate, self.coms = held.state, held.vstate, held.coms

    verify = HostCase.verify
    claim = HostCase.claim


TREE_DEPTH = 9                                  # 2^9 leaves: the depth that straddles the hand-over from the per-level kernel to the top kernel


@functools.lru_cache(maxsize=None)
def tree_levels(updated):
    """levels[0] = the 512 leaves, levels[9] = [root], node = the ORACLE's sponge over (left, right); updated: leaves 0, 257 and 511 replaced"""
    leaves = [bpg.be_to_scalar(b"\x07" + workloads.synth("walk-tree", i, 31)) for i in range(1 << TREE_DEPTH)]
    if updated:
        for i, leaf in zip(TREE_UPDATE, tree_new_leaves()):
            leaves[i] = leaf
    levels = [leaves]
    while len(levels[-1]) > 1:
        lo = levels[-1]
        levels.append([O.mimc_sponge(lo[i] + lo[i + 1]) for i in range(0, len(lo), 2)])
    return levels


TREE_UPDATE = [0, 257, 511]
TREE_PATHS = [0, 1, 255, 256, 511]


def tree_new_leaves():
    return [bpg.be_to_scalar(b"\x05" + workloads.synth("walk-tree-new", i, 31)) for i in range(len(TREE_UPDATE))]


def tree_paths(levels, indices):
    return [[levels[k][(i >> k) ^ 1] for k in range(TREE_DEPTH)] for i in indices]


# ---- the growing tree: capacity 2^11, 5 -> 6 -> 606 leaves, then four leaves replaced: the final state F, in the dense and in the prefix layout
GROW_DEPTH = 11
GROW_SIZES = (5, 6, 606)
GROW_EMPTY = rs("gtree empty", 0)               # the empty value: a fixed non-zero scalar, reduced
GROW_RESERVE = 7                                # the prefix tree's first reserve: odd; 6 leaves fit, 606 do not, and the regrow is to max(2 * 7, 606) = 606
GROW_UPDATE = [0, 5, 6, 605]                    # a leaf of the build, the leaf of the first append, the first and the last leaf of the second
GROW_PATHS = [0, 5, 6, 7, 605, 606, 607, 1024, 2047]      # occupied leaves, the first empty leaf, siblings that are empty subtrees, the far right
# What the second append launches, by plan_merkle_grow(11, 6, 606) of csrc/host/merkle_plan.hpp (tests/hostcheck/merkle_plan.cpp holds the plan to brute
# force; no Python hook exposes it): the new leaves are the heap nodes 2048 + 6 .. 2048 + 605 = 2054 .. 2653, their parents 1027 .. 1326 are 300 > 256
# nodes: ONE wide step (k_merkle_level_range; k_mpx_range at height 0) writes level 10; the parents of those, 513 .. 663, are 151 <= 256 nodes: the climb
# (k_merkle_climb / k_mpx_climb) is entered with the children of level 10 and writes level 9 and everything above.  Levels 10 and 9 are the two sides of
# that hand-over.  The build (5 leaves: parents 1024 .. 1026) and the first append (one leaf) are the fill and a climb, and a climb, only.
GROW_LEVELS = (10, 9)
assert (2048 + 605) // 2 - (2048 + 6) // 2 + 1 == 300 > 256 >= 1326 // 2 - 1027 // 2 + 1 == 151


def grow_leaves():
    return [bpg.be_to_scalar(b"\x03" + workloads.synth("walk-gtree", i, 31)) for i in range(GROW_SIZES[-1])]


def grow_new_leaves():
    return [bpg.be_to_scalar(b"\x02" + workloads.synth("walk-gtree-new", i, 31)) for i in range(len(GROW_UPDATE))]


@functools.lru_cache(maxsize=None)
def grow_empty_chain():
    """E_0 = the empty value, E_(k+1) = the ORACLE's sponge over (E_k, E_k): a subtree without a leaf, k levels above the leaves"""
    E = [GROW_EMPTY]
    for _ in range(GROW_DEPTH):
        E.append(O.mimc_sponge(E[-1] + E[-1]))
    return E


class GrowModel:
    """a sparse model of the tree that holds the first `size` leaves: heights[s] = the OCCUPIED nodes s levels above the leaves, hashed by the oracle's sponge;
    an occupied node whose right child is not occupied reads E_s, and every node that is not occupied is E_s"""
    def __init__(self, size, updated):
        leaves = grow_leaves()[:size]
        if updated:
            for i, leaf in zip(GROW_UPDATE, grow_new_leaves()):
                leaves[i] = leaf
        E = grow_empty_chain()
        self.size, self.heights = size, [leaves]
        for s in range(GROW_DEPTH):
            lo = self.heights[-1]
            self.heights.append([O.mimc_sponge(lo[2 * j] + (lo[2 * j + 1] if 2 * j + 1 < len(lo) else E[s])) for j in range((len(lo) + 1) // 2)])
        assert len(self.heights[GROW_DEPTH]) == 1

    def node(self, s, j):
        return self.heights[s][j] if j < len(self.heights[s]) else grow_empty_chain()[s]

    def root(self):
        return self.node(GROW_DEPTH, 0)

    def read(self):
        """what grow_read returns of a tree in this state"""
        D = GROW_DEPTH
        return (self.size, self.root(), list(grow_empty_chain()),
                [[self.node(k, (i >> k) ^ 1) for k in range(D)] for i in GROW_PATHS],
                [[self.node(k + 1, i >> (k + 1)) for k in range(D)] for i in GROW_PATHS],
                [[self.node(D - level, j) for j in range(1 << level)] for level in GROW_LEVELS])


@functools.lru_cache(maxsize=None)
def grow_model(size, updated):
    return GrowModel(size, updated)


def grow_read(tree):
    return (tree.size, tree.root(), tree.empty_nodes(), tree.paths(GROW_PATHS), tree.path_nodes(GROW_PATHS), [tree.nodes(level) for level in GROW_LEVELS])


def grow_final_tree(ctx):
    """F in the dense layout, built in one call over the 606 final leaves: by plan_merkle_grow(11, 0, 606) a wide step of 303 parents, then the climb"""
    leaves = grow_leaves()
    for i, leaf in zip(GROW_UPDATE, grow_new_leaves()):
        leaves[i] = leaf
    return ctx.merkle_tree(leaves, depth=GROW_DEPTH, empty=GROW_EMPTY)


def prefix_bytes(reserve):
    """32 x (sum of the stored widths W_s = max(1, ceil(reserve / 2^s)), s = 0 .. depth, + the depth + 1 constants of the empty table)"""
    return 32 * (sum(max(1, -(-reserve // (1 << s))) for s in range(GROW_DEPTH + 1)) + GROW_DEPTH + 1)


# ---- the keyed tree: depth 11, 7 -> 107 -> 122 keys, then six leaves replaced: the final state, by that history or built in one call
KEYED_DEPTH = 11
KEYED_EMPTY = rs("ktree empty", 0)              # non-zero, like GROW_EMPTY
KEYED_LEVELS = (11, 7)                          # the 2,048 leaves, and the 128 nodes of height 4, where stored nodes and empty subtrees alternate


@functools.lru_cache(maxsize=None)
def keyed_steps():
    """[(key, leaf), ...] of the build (seven keys as drawn, the last key of the tree among them), of the put of 100 new keys, of the put of 10 held and
    15 new keys, and of the update of six held keys.  Key 0 is never held."""
    draws = [k for k in KC.rand_keys(b"walk ktree", 140, KEYED_DEPTH) if k not in (0, (1 << KEYED_DEPTH) - 1)][:121]
    build = draws[:3] + [(1 << KEYED_DEPTH) - 1] + draws[3:6]
    more = draws[6:106]
    mixed = build[1:4] + draws[106:114] + more[5:12] + draws[114:121]
    update = [build[3], build[5], more[0], more[50], draws[110], draws[120]]
    leaf = lambda tag, keys: [(k, rs("ktree %s" % tag, k)) for k in keys]
    return leaf("build", build), leaf("more", more), leaf("mixed", mixed), leaf("update", update)


KEYED_ABSENT = 0
# held keys (the two ends of the tree's keys, a key of every step), absent keys beside them, the edges 0 and 2^11 - 1, the middle of the tree
KEYED_PROBE = sorted({0, 1, 1023, 1024, 2046, 2047} | {k + d for step in keyed_steps() for k, _ in (step[0], step[-1]) for d in (0, 1) if k + d < 1 << KEYED_DEPTH})


@functools.lru_cache(maxsize=None)
def keyed_model():
    """the final state, by the ORACLE's sponge: the model of tests/keyed_cases.py after the four steps"""
    m = KC.KeyedModel(KEYED_DEPTH, KEYED_EMPTY)
    for step in keyed_steps():
        m.put([k for k, _ in step], [leaf for _, leaf in step])
    held, probe = set(m.keys()), KEYED_PROBE
    assert len(held) == 122 and KEYED_ABSENT not in held and (1 << KEYED_DEPTH) - 1 in held and any(k in held for k in probe) and any(k not in held for k in probe)
    return m


def keyed_model_read():
    """what keyed_read returns of a tree in the final state"""
    m, P = keyed_model(), KEYED_PROBE
    sib = [m.siblings(i) for i in P]
    return (len(m.keys()), m.root(), list(m.E), m.keys(), m.get(P), sib, [m.on_path(i) for i in P], [bpg.merkle_path_inputs(i, s, m.root()) for i, s in zip(P, sib)],
            [m.level(level) for level in KEYED_LEVELS], m.counts())


def keyed_read(tree):
    P = KEYED_PROBE
    return (tree.size, tree.root(), tree.empty_nodes(), tree.keys(), tree.get(P), tree.paths(P), tree.path_nodes(P), tree.path_inputs(P),
            [tree.nodes(level) for level in KEYED_LEVELS], tree.node_counts[0])


def keyed_final_tree(ctx):
    """the final state built in ONE call over the 122 keys in ascending order (other capacities than the history's, the same nodes)"""
    m = keyed_model()
    return ctx.merkle_tree(m.get(m.keys())[0], depth=KEYED_DEPTH, empty=KEYED_EMPTY, keys=m.keys())


# ------------------------------------------------------------------------------------------------ the resident set of a walk
RESIDENT = {                                    # name -> how a context gets it; uploaded in this order ("b64" before "mimc": PINNED relies on it)
    "rp40": lambda ctx: ctx.upload(rp40().inst),
    "b64": lambda ctx: ctx.upload(b64(1).inst),
    "mimc": lambda ctx: ctx.upload(mimc(3).inst),
    "t_b64": lambda ctx: b64(100).prover.template(ctx),
    "t_b8": lambda ctx: b8("tmpl").prover.template(ctx),
    "t_set3": lambda ctx: mixed((("set3", 1),), "tmpl").prover.template(ctx),
    "t_chain": lambda ctx: chain(1).prover.template(ctx, param_rows=chain(1).param_rows, checkpoints=chain(1).ck_vars),
    "t_lt": lambda ctx: less_than(5, 1000, True, "walk-tmpl").prover.template(ctx),
    "tree": lambda ctx: ctx.merkle_tree(tree_levels(False)[0]),
    "t_hand": lambda ctx: hand_template().prover.template(ctx),
    "gtree": grow_final_tree,
    "ktree": keyed_final_tree,
}


class Env:
    """the context of a walk and its long-lived objects; a step names them, so a step after a free + upload gets the new handle"""
    def __init__(self, ctx):
        self.ctx, self.res, self.cap, self.pending = ctx, {}, START_CAPACITY, None
        self.model = hasattr(ctx, "model_execute")

    def setup(self):
        """the generators, the resident set, and the blinding stream that the first prove_oneshot/stream step will find begun"""
        self.ctx.gens_ensure(self.cap)
        for name in RESIDENT:
            self.res[name] = self.make(name)
        if not self.model:
            begin_stream(self)

    def make(self, name):
        return self.ctx.model_make(name) if self.model else RESIDENT[name](self.ctx)

    def reupload(self, name):
        self.res[name].free()
        self.res[name] = self.make(name)

    def grow(self):
        self.cap *= 2
        self.ctx.gens_ensure(self.cap)

    def execute(self, op):
        return self.ctx.model_execute(op, self) if self.model else op.run(self)

    def close(self):
        self.pending = None
        for h in self.res.values():
            h.free()
        self.ctx.close()


# ------------------------------------------------------------------------------------------------ operations
class Expect:
    """want: what run() must return.  claims: (HostCase, proof, status) - every proof the expectation holds and what the oracle's verifier says of it.
    checks: (instance with witness, committed values, CheckReport) - every report the expectation holds."""
    def __init__(self, want, claims=(), checks=()):
        self.want, self.claims, self.checks = want, list(claims), list(checks)


class Op:
    def __init__(self, family, variant, prepare, run, uses=(), effect=None, uploads=()):
        """uses: the resident objects run() touches (after its own effect); uploads: those it frees and uploads again; effect: what of it a model context does"""
        self.family, self.variant, self.name = family, variant, "%s/%s" % (family, variant)
        self._prepare, self.run, self.uses, self.effect, self.uploads = prepare, run, tuple(uses), effect, tuple(uploads)
        self._expect = None

    def prepare(self):
        if self._expect is None:
            self._expect = self._prepare()
        return self._expect

    @staticmethod
    def same(want, got):
        """the comparison: exact equality of everything an operation returns"""
        return want == got


CATALOGUE = {}
OPS = {}


def op(family, variant, uses=(), effect=None, uploads=()):
    """@op(family, variant): the decorated function returns (prepare, run)"""
    def register(make):
        prepare, run = make()
        o = Op(family, variant, prepare, run, uses, effect, uploads)
        CATALOGUE.setdefault(family, []).append(o)
        OPS[o.name] = o
        return o
    return register


def flipped(proof, pos):
    bad = bytearray(proof); bad[pos] ^= 1
    return bytes(bad)


# ---- 1, 2: resident proofs
def _resident_proof(family, variant, handle, case, seed_tag):
    @op(family, variant, uses=[handle])
    def _():
        seed = rng(seed_tag)

        def prepare():
            want = case().prove(seed)
            return Expect(want, [case().claim(want[0])])

        def run(env):
            c = case()
            return env.res[handle].prove(c.state, c.inst.v_blinding, seed)
        return prepare, run


_resident_proof("prove_tabled", "b64_a", "b64", lambda: b64(1), "tabled a")
_resident_proof("prove_tabled", "rp40", "rp40", rp40, "tabled rp40")
_resident_proof("prove_tabled", "b64_b", "b64", lambda: b64(1), "tabled b")
_resident_proof("prove_folded", "seed_a", "mimc", lambda: mimc(3), "folded a")
_resident_proof("prove_folded", "seed_b", "mimc", lambda: mimc(3), "folded b")


# ---- 3: one-shot proofs
def _device_prover_proof(a, seed):
    """a prover with its commitments made on the device -> (commitments, transcript after them, proof)"""
    state = a.transcript.state
    return b"".join(a.commitments), state, a.prover.prove(a.gens_capacity, seed)


@op("prove_oneshot", "prover")
def _():
    seed = rng("oneshot prover")

    def prepare():
        c = b64(5)
        want = c.prove(seed)
        return Expect((c.coms, c.state, want[0]), [c.claim(want[0])])

    def run(env):
        return _device_prover_proof(workloads.bounds_check_64(env.ctx, seed=5), seed)
    return prepare, run


@op("prove_oneshot", "flat")
def _():
    seed = rng("oneshot flat")

    def prepare():
        want = mimc(8).prove(seed)
        return Expect(want, [mimc(8).claim(want[0])])

    def run(env):
        c = mimc(8)
        return env.ctx.prove_flat(c.inst, c.state, c.inst.v_blinding, seed)
    return prepare, run


def begin_stream(env):
    """a prover whose blinding chain is started now and consumed by the NEXT prove_oneshot/stream step of this context, operations later"""
    a = workloads.bounds_check_64(env.ctx, seed=7)
    a.prover.start_blinding(rng("oneshot stream"), max_multipliers=128)
    env.pending = a


@op("prove_oneshot", "stream")
def _():
    def prepare():
        c = b64(7)
        want = c.prove(rng("oneshot stream"))
        return Expect((c.coms, c.state, want[0]), [c.claim(want[0])])

    def run(env):
        a, env.pending = env.pending, None      # (begun by Env.setup or by the step of this name before this one)
        out = _device_prover_proof(a, None)        # prove() without a seed continues with the stream's
        begin_stream(env)
        return out
    return prepare, run


# ---- 4, 5: verification
def _mangled(proof):
    """the proof, four copies with one flipped bit each, and one a byte short"""
    return [proof] + [flipped(proof, pos) for pos in (5, 100, len(proof) - 40, len(proof) - 1)] + [proof[:-1]]


def _verdicts(case, proof):
    return _mangled(proof), [case.verify(p) for p in _mangled(proof)]


@op("verify", "resident", uses=["mimc", "b64"])
def _():
    def cases():
        return [(name, c, c.prove(rng("verify resident " + name))[0]) for name, c in (("mimc", mimc(3)), ("b64", b64(1)))]

    def prepare():
        want, claims = [], []
        for _, c, proof in cases():
            proofs, st = _verdicts(c, proof)
            assert st[0] == 0 and all(st[1:])
            want.append(st); claims += [c.claim(p, s) for p, s in zip(proofs, st)]
        return Expect(want, claims)

    def run(env):
        return [[env.res[name].verify(c.state, c.coms, p) for p in _mangled(proof)] for name, c, proof in cases()]
    return prepare, run


@op("verify", "flat")
def _():
    def cases():
        return [(c, c.prove(rng("verify flat %d" % k))[0]) for k, c in enumerate((b64(2), mimc(8)))]

    def prepare():
        want, claims = [], []
        for c, proof in cases():
            proofs, st = _verdicts(c, proof)
            assert st[0] == 0 and all(st[1:])
            want.append(st); claims += [c.claim(p, s) for p, s in zip(proofs, st)]
        return Expect(want, claims)

    def run(env):
        return [[env.ctx.verify_flat(c.vinst, c.vstate, c.coms, p) for p in _mangled(proof)] for c, proof in cases()]
    return prepare, run


def _verify_batch(variant, bad_item):
    @op("verify_batch", variant, uses=["b64", "mimc"])
    def _():
        def items():
            out = []
            for k, c in enumerate((b64(1), b64(2), mimc(3), mimc(8))):
                proof = c.prove(rng("verify batch %d" % k))[0]
                out.append((c, flipped(proof, 70 + k) if k == bad_item else proof))
            return out

        def prepare():
            st = [c.verify(p) for c, p in items()]
            assert [bool(s) for s in st] == [k == bad_item for k in range(4)]
            return Expect(st, [c.claim(p, s) for (c, p), s in zip(items(), st)])

        def run(env):
            its = items()
            # two shapes; items 0 and 2 through the resident handles, 1 and 3 as verifier-side instances
            targets = [env.res["b64"], its[1][0].vinst, env.res["mimc"], its[3][0].vinst]
            return env.ctx.verify_batch([(t, c.vstate, c.coms, p) for t, (c, p) in zip(targets, its)], batch_seed=rng("batch " + variant))[0]
        return prepare, run


_verify_batch("bad_small", 1)
_verify_batch("bad_large", 2)


# ---- 6: sums
@op("sums", "msm")
def _():
    count = 190

    def scalars():
        s = [rs("ms", i) for i in range(count)]
        t = [rs("mt", i) for i in range(count)]
        for i in range(0, count, 5):
            s[i] = bytes(32)
        for i in range(1, count, 7):
            t[i] = sc(1)
        s[2] = sc(L - 1)
        return s, t

    def prepare():
        s, t = scalars()
        G, H = ogens(START_CAPACITY).export(7, count)
        return Expect(O.msm(b"".join(s + t), G + H, 1))

    def run(env):
        return env.ctx.msm_gens(7, *scalars())
    return prepare, run


@op("sums", "pedersen")
def _():
    def pairs():
        vs = [rs("pv", i) for i in range(31)] + [bytes(32), b"\xff" * 31 + b"\x7f"]
        bl = [rs("pr", i) for i in range(31)] + [bytes(32), sc(L - 1)]
        return vs, bl

    def prepare():
        return Expect([O.pedersen_commit(v, r) for v, r in zip(*pairs())])

    def run(env):
        return env.ctx.pedersen_commit(*pairs())
    return prepare, run


# ---- 7: lockstep batches of host assemblies
def _lockstep(variant, cases):
    @op("lockstep", variant)
    def _():
        def prepare():
            want = [c.prove(rng("lockstep %s %d" % (variant, k))) for k, c in enumerate(cases())]
            return Expect(want, [c.claim(w[0]) for c, w in zip(cases(), want)])

        def run(env):
            return env.ctx.prove_batch([(c.inst, c.state, c.inst.v_blinding, rng("lockstep %s %d" % (variant, k)), 0) for k, c in enumerate(cases())])
        return prepare, run


_lockstep("mixed_a", lambda: [b64(11), mimc(12), b64(13), b64(14), mimc(3)])
_lockstep("mixed_b", lambda: [mimc(8), b8("lock-0"), b8("lock-1"), mimc(12), b8("lock-2")])


# ---- 8: templates
@op("template", "assign_prove", uses=["t_b64"])
def _():
    seed = rng("template assign")

    def prepare():
        want = b64(21).prove(seed)
        return Expect(want, [b64(21).claim(want[0])])

    def run(env):
        c, t = b64(21), env.res["t_b64"]
        t.assign(c.inst.v)
        return t.prove(c.state, c.inst.v_blinding, seed)
    return prepare, run


@op("template", "batch", uses=["t_b8"])
def _():
    def cases():
        return [b8("batch-%d" % k) for k in range(5)]

    def prepare():
        want = [c.prove(rng("template batch %d" % k)) for k, c in enumerate(cases())]
        return Expect(want, [c.claim(w[0]) for c, w in zip(cases(), want)])

    def run(env):
        return env.res["t_b8"].prove_batch([(c.inst.v, [], c.state, c.inst.v_blinding, rng("template batch %d" % k), 0) for k, c in enumerate(cases())])
    return prepare, run


@op("template", "batch_commit", uses=["t_b64"])
def _():
    def cases():
        return [b64(s) for s in (22, 23, 24)]

    def prepare():
        want = [c.prove(rng("template commit %d" % k)) + (c.coms,) for k, c in enumerate(cases())]
        return Expect(want, [c.claim(w[0]) for c, w in zip(cases(), want)])

    def run(env):
        pre = state_before(b"BoundsCheck")
        return env.res["t_b64"].prove_batch_commit([(c.inst.v, [], pre, c.inst.v_blinding, rng("template commit %d" % k), 0) for k, c in enumerate(cases())])
    return prepare, run


# ---- 9: checkpointed batches and public inputs
@op("template_ck_inputs", "ck_batch", uses=["t_chain"])
def _():
    BADK = 2

    def items():
        out = []
        for k in range(4):
            c = chain(2 + k)
            ck = list(c.ck_values)
            if k == BADK:                       # checkpoints 1 and 4 wrong: the lowest is reported
                ck[1] = sc(int.from_bytes(ck[1], "little") + 1); ck[4] = sc(int.from_bytes(ck[4], "little") + 1)
            out.append((c, (c.inst.v, c.params, c.state, c.inst.v_blinding, rng("ck batch %d" % k), 0, ck)))
        return out

    def prepare():
        res, claims = [], []
        for k, (c, _) in enumerate(items()):
            if k == BADK:
                res.append((None, c.state))     # a failed item's transcript is left as given
            else:
                res.append(c.prove(rng("ck batch %d" % k))); claims.append(c.claim(res[-1][0]))
        return Expect((res, [ERR_MISMATCH if k == BADK else 0 for k in range(4)], [1 if k == BADK else None for k in range(4)]), claims)

    def run(env):
        return env.res["t_chain"].prove_batch_checkpointed([it for _, it in items()], return_status=True)
    return prepare, run


@op("template_ck_inputs", "inputs_commit", uses=["t_lt"])
def _():
    PAIRS = [(10, 500), (2**125 - 3, 2**126 - 1), (0, 1), (77, 5000)]

    def cases():
        return [less_than(left, bound, False, "walk-%d" % k) for k, (left, bound) in enumerate(PAIRS)]

    def prepare():
        want = [c.prove(rng("inputs %d" % k)) + (c.coms,) for k, c in enumerate(cases())]
        return Expect(want, [c.claim(w[0]) for c, w in zip(cases(), want)])

    def run(env):
        pre = state_before(b"LessThan")
        return env.res["t_lt"].prove_batch_inputs([(c.inst.v, [], pre, c.inst.v_blinding, rng("inputs %d" % k), 0, None, [TC.sc(PAIRS[k][1])])
                                                   for k, c in enumerate(cases())], commit=True)
    return prepare, run


# ---- 10: repeat, join, check
@op("repeat_join_check", "repeat", uses=["t_b8"])
def _():
    seed = rng("repeat")

    def prepare():
        want = b8("rep", 3).prove(seed)
        return Expect(want, [b8("rep", 3).claim(want[0])])

    def run(env):
        c = b8("rep", 3)
        rep = env.res["t_b8"].repeat(3)
        try:
            rep.assign(c.inst.v, c.params)
            return rep.prove(c.state, c.inst.v_blinding, seed)
        finally:
            rep.free()
    return prepare, run


@op("repeat_join_check", "join", uses=["t_set3", "t_b8"])
def _():
    seed = rng("join")
    PARTS = (("set3", 2), ("bounds8", 3))

    def prepare():
        want = mixed(PARTS, "join").prove(seed)
        return Expect(want, [mixed(PARTS, "join").claim(want[0])])

    def run(env):
        c = mixed(PARTS, "join")
        j = env.ctx.join([(env.res["t_set3"], 2), (env.res["t_b8"], 3)])
        try:
            j.assign(c.inst.v, c.params)
            return j.prove(c.state, c.inst.v_blinding, seed)
        finally:
            j.free()
    return prepare, run


def _values(c):
    return [c.inst.v[32 * i:32 * i + 32] for i in range(c.inst.m)]


@op("repeat_join_check", "check", uses=["t_b8", "mimc"])
def _():
    def cases():
        return [b8("chk-0"), b8("chk-1"), b8("chk-2", 1, bad_item=0), b8("chk-3")]

    def other_values():
        """the committed values of the resident MiMC circuit with the first one raised by one: the rows that name it break"""
        v = mimc(3).inst.v
        return sc(int.from_bytes(v[:32], "little") + 1) + v[32:]

    def prepare():
        cs, big = cases(), mimc(3)
        reports = [bpg.test_check_host(c.inst) for c in cs]
        assert [r.ok for r in reports] == [True, True, False, True] and reports[2].bad_multipliers == 0
        good, bad = bpg.test_check_host(big.inst), bpg.test_check_host(big.inst, other_values())
        assert good.ok and bad.bad_rows > 0 and bad.bad_multipliers == 0
        return Expect((reports[2], reports[0], [r.rows for r in reports], good, bad),
                      checks=[(c.inst, c.inst.v, r) for c, r in zip(cs, reports)] + [(big.inst, big.inst.v, good), (big.inst, other_values(), bad)])

    def run(env):
        cs, t = cases(), env.res["t_b8"]
        t.assign(cs[2].inst.v)
        bad = t.check()
        t.assign(cs[0].inst.v)
        # ... and on the plain upload that the proofs around this step are of: its row view is built here, between two of them
        return bad, t.check(), t.check_batch([(_values(c), b"") for c in cs]), env.res["mimc"].check(mimc(3).inst.v), env.res["mimc"].check(other_values())
    return prepare, run


@op("repeat_join_check", "repeat_inputs")
def _():
    seed = rng("repeat inputs")

    def prepare():
        want = inequality3().prove(seed)
        return Expect(want, [inequality3().claim(want[0])])

    def run(env):
        c = inequality3()
        tmpl = inequality_template().prover.template(env.ctx)
        try:
            rep = tmpl.repeat_inputs(3)
        finally:
            tmpl.free()                         # the source goes before the repeat is first used
        try:
            rep.assign(c.inst.v, c.params, inputs=c.inputs)         # three witnesses against three public values, item-major
            return rep.prove(c.state, c.inst.v_blinding, seed)
        finally:
            rep.free()
    return prepare, run


# ---- 11: Merkle trees and sponges
def _tree_op(variant, updated, act, **kw):
    @op("merkle", variant, uses=["tree"], **kw)
    def _():
        def prepare():
            levels = tree_levels(updated)
            return Expect((levels[-1][0], tree_paths(levels, TREE_PATHS)))

        def run(env):
            act(env)
            tree = env.res["tree"]
            return tree.root(), tree.paths(TREE_PATHS)
        return prepare, run


_tree_op("build", False, lambda env: env.reupload("tree"), effect=lambda env: env.reupload("tree"), uploads=["tree"])                                        # a fresh tree over the original leaves
_tree_op("update", True, lambda env: env.res["tree"].update(TREE_UPDATE, tree_new_leaves()))        # (the same three leaves every time: idempotent)


@op("merkle", "sponges")
def _():
    def items():
        return [rs("sponge", 2 * k) + rs("sponge", 2 * k + 1) for k in range(65)]

    def prepare():
        return Expect([O.mimc_sponge(it) for it in items()])

    def run(env):
        return env.ctx.mimc_sponge_many(items(), 2)
    return prepare, run


# ---- 12: lifecycle
def _reupload(name, other, prepare, run):
    """free + upload of `name`; what the step returns is a proof on `other`, which was uploaded before it: the new handle's first use is a later step's"""
    op("lifecycle", "reupload_" + name, uses=[other], uploads=[name], effect=lambda env: env.reupload(name))(
        lambda: (prepare, lambda env: (env.reupload(name), run(env))[1]))


def _reupload_circuit(name, other, case, tag):
    def prepare():
        want = case().prove(rng(tag))
        return Expect(want, [case().claim(want[0])])
    _reupload(name, other, prepare, lambda env: env.res[other].prove(case().state, case().inst.v_blinding, rng(tag)))


_reupload_circuit("mimc", "b64", lambda: b64(1), "reupload mimc")


@op("lifecycle", "grow", effect=lambda env: env.grow())
def _():
    def prepare():
        return Expect(ogens(START_CAPACITY).export(1000, 24))

    def run(env):
        env.grow()
        return env.ctx.gens_export(1000, 24)
    return prepare, run


_reupload_circuit("b64", "rp40", rp40, "reupload b64")


def _reupload_template():
    def prepare():
        want = b64(25).prove(rng("reupload t_b8"))
        return Expect(want, [b64(25).claim(want[0])])

    def run(env):
        c, t = b64(25), env.res["t_b64"]
        t.assign(c.inst.v)
        return t.prove(c.state, c.inst.v_blinding, rng("reupload t_b8"))
    _reupload("t_b8", "t_b64", prepare, run)


_reupload_template()


# ---- 13: refusals that leave nothing behind
@op("refusal", "invalid_argument")
def _():
    def prepare():
        return Expect((ERR_INVALID, b"\xa5" * 32))

    def run(env):
        out = C.create_string_buffer(b"\xa5" * 32, 32)          # a range beyond any capacity: refused before the device is touched, nothing written
        st = bpg.lib().bpg_msm_gens(env.ctx._h, C.c_uint64(1 << 24), C.c_uint64(1), sc(1), sc(1), out)
        return st, out.raw
    return prepare, run


@op("refusal", "unsatisfied_item", uses=["t_b8"])
def _():
    def cases():
        return [b8("unsat-0"), b8("unsat-1", 1, bad_item=0), b8("unsat-2")]

    def prepare():
        # a witness that breaks the circuit is proved all the same (the prover does not judge it): the oracle's bytes, and a proof nobody accepts
        want = [c.prove(rng("unsat %d" % k)) for k, c in enumerate(cases())]
        verdicts = [c.verify(w[0]) for c, w in zip(cases(), want)]
        assert verdicts == [0, 3, 0]
        return Expect((want, [0, 0, 0], verdicts), [c.claim(w[0], s) for c, w, s in zip(cases(), want, verdicts)])

    def run(env):
        cs = cases()
        res, st = env.res["t_b8"].prove_batch([(c.inst.v, [], c.state, c.inst.v_blinding, rng("unsat %d" % k), 0) for k, c in enumerate(cs)], return_status=True)
        verdicts = env.ctx.verify_batch([(c.inst, c.state, c.coms, r[0]) for c, r in zip(cs, res)], batch_seed=rng("unsat batch"))[0]
        return res, st, verdicts
    return prepare, run


def _lost_upload(variant, hook, word):
    @op("refusal", variant, uses=["mimc"])
    def _():
        seed = rng("refusal " + variant)

        def prepare():
            return Expect((ERR_DEVICE, True))

        def run(env):
            c = mimc(3)
            assert getattr(bpg.lib(), hook)(env.ctx._h) == 0
            env.ctx.blinding_begin(c.state, c.inst.v_blinding, seed, c.inst.n)
            try:
                env.res["mimc"].prove(c.state, c.inst.v_blinding, seed)
            except bpg.BpgError as e:
                return e.status, word in str(e)
            return 0, False
        return prepare, run


_lost_upload("fail_upload", "bpg_test_fail_next_upload", "upload")       # the upload of the stream's first block reports an error
_lost_upload("drop_upload", "bpg_test_drop_next_upload", "stale")        # the copies are skipped without one: the slab's canary withholds the proof


# ---- 14: a growing tree, dense and prefix layout: every mutating variant ends in the same final state F
def _grow_rebuild(env, reserve):
    """free + build over 5 leaves + append 1 + append 600 + the update -> (what the appends returned, the reserve in between and at the end)"""
    leaves = grow_leaves()
    env.res["gtree"].free()
    tree = env.res["gtree"] = env.ctx.merkle_tree(leaves[:GROW_SIZES[0]], depth=GROW_DEPTH, empty=GROW_EMPTY, reserve=reserve)
    appended = [tree.append(leaves[GROW_SIZES[0]:GROW_SIZES[1]], return_root=True)]
    held = [tree.reserved] if reserve else []
    appended.append(tree.append(leaves[GROW_SIZES[1]:GROW_SIZES[2]], return_root=True))
    tree.update(GROW_UPDATE, grow_new_leaves())
    if reserve:
        tree.reserve(GROW_SIZES[1])             # room there is already: a reserve never shrinks
        held.append(tree.reserved)
    return appended, held


def _grow_op(variant, reserve, held):
    @op("merkle_grow", variant, uses=["gtree"], uploads=["gtree"], effect=lambda env: env.reupload("gtree"))
    def _():
        def prepare():
            appended = [(GROW_SIZES[k], grow_model(GROW_SIZES[k + 1], False).root()) for k in range(2)]
            return Expect((appended, held, grow_model(GROW_SIZES[2], True).read()))

        def run(env):
            appended, got = _grow_rebuild(env, reserve)
            return appended, got, grow_read(env.res["gtree"])
        return prepare, run


_grow_op("dense", None, [])
# the first append fits the reserve of 7; the second regrows to exactly 606, where the stored width of height 1 is 303, odd: node (2, 151) reads its
# right child from the empty table
_grow_op("prefix", GROW_RESERVE, [(GROW_RESERVE, prefix_bytes(GROW_RESERVE)), (GROW_SIZES[2], prefix_bytes(GROW_SIZES[2]))])


@op("merkle_grow", "read", uses=["gtree"])
def _():
    def prepare():
        return Expect(grow_model(GROW_SIZES[2], True).read())

    def run(env):
        tree = env.res["gtree"]                 # in whichever layout the last rebuild left it
        tree.update(GROW_UPDATE, grow_new_leaves())         # (the same four leaves every time: idempotent)
        return grow_read(tree)
    return prepare, run


# ---- 15: a gated template: ONE circuit for every input vector; every expectation is the oracle's proof of the ungated yardstick
def _hand_seed(k):
    return rng("gates vector %d" % k)


@op("gates", "assign_prove", uses=["t_hand"])
def _():
    ORDER = (1, 2, 3, 0)

    def other(k):
        """the statement of the NEXT vector's inputs claimed for vector k's commitments"""
        return Crossed(hand(GC.HAND_INPUTS[(k + 1) % 4], GC.HAND_VALUES[k]), hand_vector(k))

    def prepare():
        want, claims = [], []
        for k in ORDER:
            c = hand_vector(k)
            proof, after = c.prove(_hand_seed(k))
            st = (c.verify(proof), other(k).verify(proof))
            assert st == (0, 3)
            want.append((True, proof, after) + st)
            claims += [c.claim(proof), other(k).claim(proof, 3)]
        return Expect(want, claims)

    def run(env):
        t, out = env.res["t_hand"], []
        for k in ORDER:
            c = hand_vector(k)
            t.assign(c.inst.v, inputs=hand_inputs(k))
            ok = t.check().ok
            proof, after = t.prove(c.state, c.inst.v_blinding, _hand_seed(k))
            good = t.verify(c.state, c.coms, proof)
            t.set_inputs(hand_inputs((k + 1) % 4))          # the verifier's half: other inputs, another statement
            out.append((ok, proof, after, good, t.verify(c.state, c.coms, proof)))
        t.set_inputs(hand_inputs(ORDER[-1]))                # the standing slots are this variant's own last inputs, whatever ran before
        return out
    return prepare, run


@op("gates", "wave", uses=["t_hand"])
def _():
    K = 65                                      # item 64: one past a 64-lane block

    def inputs(k):
        return ((7 * k + 1) * 2 ** (3 * k % 250) % L, k % 2, L - 1 - k, 2 ** 252 + 9 + k)

    def cases():
        return [hand(inputs(k), ((k + 2) % L, (L - 5 * k - 1) % L), "b%d" % k) for k in range(K)]

    def prepare():
        cs = cases()
        proofs = [c.prove(rng("gates wave %d" % k)) for k, c in enumerate(cs)]
        return Expect((proofs, [p + (c.coms,) for p, c in zip(proofs, cs)]), [c.claim(p[0]) for c, p in zip(cs, proofs)])

    def run(env):
        pre, out = state_before(b"hand10"), []
        for commit in (False, True):
            items = [(c.inst.v, [], pre if commit else c.state, c.inst.v_blinding, rng("gates wave %d" % k), 0, None, [sc(x) for x in inputs(k)])
                     for k, c in enumerate(cases())]
            out.append(env.res["t_hand"].prove_batch_inputs(items, commit=commit))
        return tuple(out)
    return prepare, run


@op("gates", "check", uses=["t_hand"])
def _():
    VECTOR = 2                                  # inputs (2^252 + 9, l - 1, 0, 1): the gated term 5 x_2 v_1 of row 7 is switched off

    def other_values():
        """the witness of vector 2 with its second committed value raised by one.  assign() computes every multiplier from the committed values, so no
        assign can break a row of this circuit (no row ties a multiplier to anything but the terms it is computed from): a row breaks where the committed
        values are not the ones the multipliers were computed from, which is what check(values) is given"""
        v = hand_vector(VECTOR).inst.v
        return v[:32] + sc(int.from_bytes(v[32:64], "little") + 1)

    def prepare():
        c = hand_vector(VECTOR)
        good, bad = bpg.test_check_host(c.inst), bpg.test_check_host(c.inst, other_values())
        assert good.ok and bad.bad_multipliers == 0 and bad.rows == [0, 5]     # the rows that name v_1 under a coefficient that is not zero
        return Expect((bad, bad.rows, good, good.rows), checks=[(c.inst, c.inst.v, good), (c.inst, other_values(), bad)])

    def run(env):
        c, t = hand_vector(VECTOR), env.res["t_hand"]
        t.assign(c.inst.v, inputs=hand_inputs(VECTOR))
        bad = t.check(other_values())
        t.assign(c.inst.v, inputs=hand_inputs(VECTOR))
        good = t.check()
        return bad, bad.rows, good, good.rows
    return prepare, run


# ---- 16: lockstep verification on one resident circuit.  Verdicts are the oracle verifier's.  The state after an item is the state after the oracle's
# proof wherever the verifier replays what the prover absorbed: every commitment of the proof and t_x, t_x_blinding, e_blinding, but neither of the last two
# scalars a and b, and nothing of the circuit's constants - so also for a proof with a changed a and for a good proof under wrong constants
def _wave_seed(k):
    return rng("verify wave item %d" % k)


@op("verify_wave", "plain", uses=["b64"])
def _():
    TRUNCATED = 4

    def items():
        c = b64(1)
        good = [c.prove(rng("verify wave plain %d" % k)) for k in range(3)]
        bad = flipped(good[1][0], len(good[1][0]) - 40)            # byte 24 of a
        return c, [good[0], (bad, good[1][1]), good[1], good[2], (good[0][0][:-1], None)]

    def prepare():
        c, its = items()
        st = [c.verify(p) for p, _ in its]
        assert st == [0, 3, 0, 0, 2]
        return Expect((st, [after for k, (_, after) in enumerate(its) if k != TRUNCATED]), [c.claim(p, s) for (p, _), s in zip(its, st)])

    def run(env):
        c, its = items()
        st, states = env.res["b64"].verify_batch([(c.state, c.coms, p, _wave_seed(k)) for k, (p, _) in enumerate(its)], batch_seed=rng("verify wave plain"))
        return st, [s for k, s in enumerate(states) if k != TRUNCATED]
    return prepare, run


@op("verify_wave", "inputs", uses=["t_lt"])
def _():
    PAIRS = [(10, 500), (2**125 - 3, 2**126 - 1), (0, 1), (77, 5000)]          # the statements (and so the cached proofs) of template_ck_inputs/inputs_commit
    STANDING = 2                                # the bound that stands in the circuit while the wave runs; the wave's LAST item brings another

    def cases():
        return [less_than(left, bound, False, "walk-%d" % k) for k, (left, bound) in enumerate(PAIRS)]

    def items():
        """(the statement a verifier with these inputs judges, the bound it is given, the proof, the state after)"""
        cs = cases()
        out = [(c, PAIRS[k][1]) + c.prove(rng("inputs %d" % k)) for k, c in enumerate(cs)]
        return out + [(Crossed(cs[3], cs[0]), PAIRS[3][1]) + cs[0].prove(rng("inputs 0"))]      # a good proof and the wrong bound

    def standing():
        """two proofs judged alone under the standing bound: the one made against it, and another"""
        cs = cases()
        return [(cs[STANDING], cs[STANDING].prove(rng("inputs %d" % STANDING))[0]), (Crossed(cs[STANDING], cs[3]), cs[3].prove(rng("inputs 3"))[0])]

    def prepare():
        st = [c.verify(proof) for c, _, proof, _ in items()]
        alone = [c.verify(proof) for c, proof in standing()]
        assert st == [0, 0, 0, 0, 3] and alone == [0, 3]
        return Expect((alone, st, [after for _, _, _, after in items()], alone),
                      [c.claim(proof, s) for (c, _, proof, _), s in zip(items(), st)] + [c.claim(proof, s) for (c, proof), s in zip(standing(), alone)])

    def run(env):
        t = env.res["t_lt"]
        t.set_inputs([TC.sc(PAIRS[STANDING][1])])
        alone = lambda: [t.verify(c.state, c.coms, proof) for c, proof in standing()]
        before = alone()
        st, states = t.verify_batch([(c.state, c.coms, proof, _wave_seed(k), 0, None, [TC.sc(bound)]) for k, (c, bound, proof, _) in enumerate(items())],
                                    batch_seed=rng("verify wave inputs"))
        return before, st, states, alone()      # the wave must not have written the circuit's table
    return prepare, run


@op("verify_wave", "gated", uses=["t_hand"])
def _():
    def items():
        """(the statement, the vector whose inputs the item brings, the proof, the state after)"""
        out = [(hand_vector(k), k) + hand_vector(k).prove(_hand_seed(k)) for k in range(4)]
        return out + [(Crossed(hand(GC.HAND_INPUTS[2], GC.HAND_VALUES[1]), hand_vector(1)), 2) + hand_vector(1).prove(_hand_seed(1))]

    def prepare():
        st = [c.verify(proof) for c, _, proof, _ in items()]
        assert st == [0, 0, 0, 0, 3]
        return Expect((st, [after for _, _, _, after in items()]), [c.claim(proof, s) for (c, _, proof, _), s in zip(items(), st)])

    def run(env):
        return env.res["t_hand"].verify_batch([(c.state, c.coms, proof, _wave_seed(k), 0, None, hand_inputs(v)) for k, (c, v, proof, _) in enumerate(items())],
                                              batch_seed=rng("verify wave gated"))
    return prepare, run


# ---- 17: a keyed tree: every mutating variant ends in the same final state; expectations from keyed_cases.KeyedModel (the oracle's sponge, memoised)
def _keyed_rebuild(env):
    """free + build over seven unsorted keys + 100 new keys (arrays retired and replaced) + 25 mixed keys (merged in the scratch) + the update
    -> (the keys each put inserted, the root after each step, node_counts at the end)"""
    env.res["ktree"].free()
    steps = keyed_steps()
    tree = env.res["ktree"] = env.ctx.merkle_tree([leaf for _, leaf in steps[0]], depth=KEYED_DEPTH, empty=KEYED_EMPTY, keys=[k for k, _ in steps[0]])
    inserted, roots = [], [tree.root()]
    for step in steps[1:3]:
        n, root = tree.put([k for k, _ in step], [leaf for _, leaf in step], return_root=True)
        inserted.append(n); roots.append(root)
    tree.update([k for k, _ in steps[3]], [leaf for _, leaf in steps[3]])
    roots.append(tree.root())
    return inserted, roots, tree.node_counts


@op("merkle_keyed", "rebuild", uses=["ktree"], uploads=["ktree"], effect=lambda env: env.reupload("ktree"))
def _():
    def prepare():
        m, inserted, roots, caps = KC.KeyedModel(KEYED_DEPTH, KEYED_EMPTY), [], [], [0] * (KEYED_DEPTH + 1)
        kinds = []
        for step in keyed_steps():
            before = m.counts()
            inserted.append(m.put([k for k, _ in step], [leaf for _, leaf in step])[0])
            roots.append(m.root())
            kind, caps = KC.merge_kinds(caps, before, m.counts(), KEYED_DEPTH)
            kinds.append(kind[0])
        # what the steps are for: the 100 new keys outgrow the minimum capacity at the leaves, the 25 mixed keys fit the room that made, the update inserts nothing
        assert kinds == ["grows", "grows", "in place", None] and inserted == [7, 100, 15, 0] and caps[0] == 2 * KC.MIN_CAPACITY
        assert roots[-1] == keyed_model().root() and m.counts() == keyed_model().counts()
        return Expect((inserted[1:3], roots, (m.counts(), 36 * sum(caps) + 32 * (KEYED_DEPTH + 1)), keyed_model_read()))

    def run(env):
        return _keyed_rebuild(env) + (keyed_read(env.res["ktree"]),)
    return prepare, run


@op("merkle_keyed", "refuse", uses=["ktree"])
def _():
    def calls(tree):
        absent, held = KEYED_ABSENT, keyed_steps()[3][0][0]
        return [lambda: tree.update([held, absent], [sc(1), sc(2)]),            # refused after the structure of height 0 ran: a key that is not held
                lambda: tree.put([held, absent, held], [sc(1), sc(2), sc(3)]),  # a key given twice
                lambda: tree.put([absent, 1 << KEYED_DEPTH], [sc(1), sc(2)])]   # a key of 2^depth

    def prepare():
        return Expect(([ERR_INVALID] * 3, keyed_model_read()))

    def run(env):
        tree, st = env.res["ktree"], []
        for call in calls(tree):
            try:
                call()
                st.append(0)
            except bpg.BpgError as e:
                st.append(e.status)
        return st, keyed_read(tree)
    return prepare, run


@op("merkle_keyed", "read", uses=["ktree"])
def _():
    def prepare():
        return Expect(keyed_model_read())

    def run(env):
        tree = env.res["ktree"]
        tree.update([k for k, _ in keyed_steps()[3]], [leaf for _, leaf in keyed_steps()[3]])      # (the same six leaves every time: idempotent)
        return keyed_read(tree)
    return prepare, run


FAMILIES = list(CATALOGUE)
assert len(FAMILIES) == 17


# ------------------------------------------------------------------------------------------------ walks
def variant_of(family, k, grows=0):
    """the variant of the k-th occurrence of a family: in rotation; lifecycle/grow only while the generators may still grow"""
    ops = CATALOGUE[family]
    if family == "lifecycle":
        ops = [o for o in ops if o.variant != "grow" or grows < MAX_GROWS]
    return ops[k % len(ops)]


def with_variants(families):
    seen, grows, steps = {}, 0, []
    for f in families:
        o = variant_of(f, seen.get(f, 0), grows)
        seen[f] = seen.get(f, 0) + 1
        grows += o.variant == "grow"
        steps.append((o.family, o.variant))
    return steps


def build_walk(seed):
    """An Eulerian circuit of the complete directed graph on the families with a loop at every one (in-degree = out-degree = 17 everywhere, so one exists):
    randomised Hierholzer.  17 x 17 edges -> 290 steps in which every ordered pair of families, a family after itself included, is adjacent exactly once."""
    rnd = random.Random(seed)
    out = {f: rnd.sample(FAMILIES, len(FAMILIES)) for f in FAMILIES}         # the unused edges f -> g, in the order they will be taken
    stack, circuit = [rnd.choice(FAMILIES)], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return with_variants(circuit)


PINNED = [
    ("the tables of the original generators, kept from proof to proof, against the tables of folded generators that live in the arena",
     ["prove_tabled/rp40", "prove_folded/seed_a", "prove_tabled/rp40", "prove_folded/seed_b"]),
    ("a verification's one sum over the arena and a lockstep wave's buffers between two proofs of one circuit",
     ["prove_folded/seed_a", "verify/resident", "lockstep/mixed_a", "prove_folded/seed_b"]),
    ("the row view of check() built between two proofs: no byte changes",
     ["prove_folded/seed_a", "repeat_join_check/check", "prove_folded/seed_a"]),
    ("a tree's leaf update and root after a proof used the arena",
     ["merkle/build", "prove_folded/seed_a", "merkle/update"]),
    ("generators that grow between an upload and its first proof (the step that uploads proves another circuit)",
     ["lifecycle/reupload_mimc", "lifecycle/grow", "prove_folded/seed_a"]),
    ("generators that grow before the first use of anything in the resident set",
     ["lifecycle/grow", "prove_folded/seed_a", "prove_tabled/rp40", "template/assign_prove", "merkle/update"]),
    ("a withheld proof leaves the blinding slab and its canary fit for the next two",
     ["refusal/drop_upload", "prove_oneshot/stream", "prove_oneshot/flat"]),
    ("a batch with a failed item before a batch verification",
     ["template_ck_inputs/ck_batch", "verify_batch/bad_small"]),
    ("a circuit freed and uploaded again, then a proof of one that was uploaded before it",
     ["lifecycle/reupload_mimc", "prove_tabled/b64_a"]),
    ("a relayout's new buffer (the old one freed in the middle of an append) and the arena of a folded proof, then the tree read again",
     ["merkle_grow/prefix", "prove_folded/seed_a", "merkle_grow/read"]),
    ("tables swapped under a growing tree and a gated template before either is touched",
     ["lifecycle/grow", "merkle_grow/read", "gates/wave"]),
    ("two trees on one pair of staging buffers (mk_in / mk_out): the lists of an update and the paths of the other tree in between",
     ["merkle/update", "merkle_grow/read", "merkle/update"]),
    ("standing slots of one template between a verification wave with per-item inputs and a proving wave",
     ["verify_wave/inputs", "template_ck_inputs/inputs_commit", "verify_wave/inputs"]),
    ("lv / rv and the arena sized by a verification wave between two proofs that sized them too",
     ["prove_folded/seed_a", "verify_wave/plain", "prove_folded/seed_b"]),
    ("coefficient class 3 (a gated two-slot term in the packed stream) between waves that never saw that class",
     ["gates/wave", "lockstep/mixed_a", "gates/assign_prove"]),
    ("a keyed rebuild behind a prefix rebuild: the put stages its leaves in mk_in and exports its roots through mk_out right after an append used both, and its hashing follows k_mpx_* in the tree-hashing profile slots",
     ["merkle_grow/prefix", "merkle_keyed/rebuild", "merkle_grow/read", "merkle_keyed/read"]),
    ("a keyed rebuild ahead of a prefix rebuild: the append finds mk_in and mk_out as the put's leaves, paths and levels left them, and both trees are read again",
     ["merkle_keyed/rebuild", "merkle_grow/prefix", "merkle_keyed/read", "merkle_grow/read"]),
    ("a refused update stops after the structure of height 0 wrote the dirty list, the flags, the tile sums and the totals: the next put trusts none of it, and a folded proof takes the arena in between",
     ["merkle_keyed/refuse", "merkle_keyed/read", "prove_folded/seed_a", "merkle_keyed/rebuild", "merkle_keyed/refuse", "merkle_keyed/read"]),
    ("the scratch of a keyed put (mkx_dirty .. mkx_merge) sized by a rebuild, then a put of one tile into it after the dense tree's update went through the shared mk_in / mk_out",
     ["merkle_keyed/rebuild", "merkle/update", "merkle_keyed/read", "merkle_keyed/rebuild"]),
]

# orders for TWO contexts of one device (step i goes to context i mod 2)
PINNED_TWO = [
    ("a keyed rebuild dealt to the second context: every context has put scratch of its own, and the first context's tree, last touched before the other's rebuild, reads back unchanged",
     ["merkle_keyed/read", "merkle_keyed/rebuild", "merkle_keyed/read", "merkle_keyed/read", "merkle_grow/read", "merkle_keyed/refuse", "merkle_keyed/read", "merkle_keyed/rebuild"]),
]


def first_used_after_a_grow(names):
    """the resident objects whose first use after an upload (the resident set's, or a later free + upload) came after a grow of the generators that
    followed that upload, as (name, index of the upload or -1, index of the grow, index of the use); one context"""
    fresh, out = {name: (-1, None) for name in RESIDENT}, []        # name -> (where it was uploaded, the first grow since), until its first use
    for i, n in enumerate(names):
        o = OPS[n]
        for name in o.uploads:
            fresh[name] = (i, None)
        for name in o.uses:
            if name in fresh:
                up, grew = fresh.pop(name)
                if grew is not None:
                    out.append((name, up, grew, i))
        if o.name == "lifecycle/grow":
            fresh = {name: (up, i if grew is None else grew) for name, (up, grew) in fresh.items()}
    return out


# ------------------------------------------------------------------------------------------------ runner
class WalkMismatch(AssertionError):
    def __init__(self, index, name, done, what):
        self.index, self.op, self.steps = index, name, list(done)
        super().__init__("step %d (%s): %s\nreplay(%r)" % (index, name, what, self.steps))


def _name(step):
    return step if isinstance(step, str) else "%s/%s" % step


def run_walk(ctx_factory, steps, contexts=1, census=None, observe=None):
    """Run the steps (names or (family, variant) pairs) on `contexts` fresh contexts of ctx_factory, step i on context i mod contexts, each with a resident
    set of its own, and compare after every step.  No retry, no shrinking.  At the end everything is freed and the contexts are closed: the census of what
    the process holds must be what it was before they were made.  observe(env, index, name) is called after every step that passed, and as (env, -1, "setup") when a context has its resident set."""
    census = census or bpg.live_resources
    names = [_name(s) for s in steps]
    expects = [OPS[n].prepare() for n in names]                 # every expectation before the first context exists
    gc.collect()                                                # the census is the process's: what earlier callers dropped without freeing goes now, not during the walk
    before = census()
    envs, done = [], []
    try:
        for _ in range(contexts):
            envs.append(Env(ctx_factory()))
            envs[-1].setup()
            if observe is not None:
                observe(envs[-1], -1, "setup")
        for i, (name, exp) in enumerate(zip(names, expects)):
            done.append(name)
            try:
                got = envs[i % contexts].execute(OPS[name])
            except Exception as e:      # noqa: BLE001
                raise WalkMismatch(i, name, done, "raised %r" % (e,)) from e
            if not Op.same(exp.want, got):
                raise WalkMismatch(i, name, done, "the result differs from the expectation\n  want %s\n  got  %s" % (_short(exp.want), _short(got)))
            if observe is not None:
                observe(envs[i % contexts], i, name)
    finally:
        for env in envs:
            env.close()
    gc.collect()
    after = census()
    if after != before:
        raise WalkMismatch(len(names), "close", done, "something is left behind: the census was %r and is %r" % (before, after))


def replay(names, ctx_factory=None, contexts=1):
    run_walk(ctx_factory or (lambda: bpg.Context(0)), names, contexts)


def _short(x, limit=600):
    def show(v):
        if isinstance(v, (bytes, bytearray)):
            return "%s..(%d bytes, sha256 %s)" % (bytes(v[:8]).hex(), len(v), hashlib.sha256(v).hexdigest()[:12])
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(show(y) for y in v) + "]"
        return repr(v)
    s = show(x)
    return s if len(s) <= limit else s[:limit] + " ..."


# ------------------------------------------------------------------------------------------------ a model context (tests/test_context_walk_host.py)
class ModelHandle:
    def __init__(self, name):
        self.name, self.freed, self.frees = name, False, 0

    def free(self):
        self.freed, self.frees = True, self.frees + 1


class ModelWorld:
    """the census of a process that holds model contexts only"""
    def __init__(self):
        self.buffers = 0

    def census(self):
        return {"device_buffers": self.buffers}


class ModelContext:
    """A pure-Python stand-in for a context whose operations return the expectations: the walk harness run without a device.  It keeps the lifetimes of the
    resident set (a step that names a freed handle is an error) and counts a buffer per live handle and one for itself."""
    def __init__(self, world):
        self.world, self.capacity, self.handles, self.closed = world, 0, [], False
        world.buffers += 1

    def gens_ensure(self, capacity):
        assert capacity >= self.capacity and capacity & (capacity - 1) == 0
        self.capacity = capacity

    def model_make(self, name):
        h = ModelHandle(name)
        self.handles.append(h)
        self.world.buffers += 1
        return h

    def truth(self, op, env):
        assert not self.closed
        for name in op.uses:
            assert not env.res[name].freed, "%s uses the freed handle %s" % (op.name, name)
        if op.effect is not None:
            op.effect(env)
        return copy.deepcopy(op.prepare().want)

    def model_execute(self, op, env):
        return self.truth(op, env)

    def close(self):
        self.closed = True
        self.world.buffers -= 1 + sum(h.frees == 1 for h in self.handles)
