"""Circuits with a PUBLIC side for the tests of public inputs in circuit templates (tests/test_template_inputs_host.py, tests/test_template_inputs_gpu.py).

Every builder assembles ONE statement twice over, as the issue's yardstick needs it: as_inputs=True hands the public values to Prover.input and names the
variables; as_inputs=False bakes the same values in as constants - the host assembly every proof of a template with inputs must equal byte for byte.
Seeds, blindings and values are pinned: nothing here is random.

A Case carries what both test files read: the prover, its transcript, the commitments (empty for a device-less prover), the committed values and the
public inputs in input order."""
import hashlib

import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads

L = bpg.L
sc = lambda x: (x % (1 << 256)).to_bytes(32, "little")


def blind(tag, i):
    return workloads.blinding("template-inputs-" + tag, i)


def rng(tag):
    return hashlib.sha256(("template inputs %s" % tag).encode()).digest()


class StubProver(bpg.Prover):
    """Assembly-only prover; commitments are hash bytes made on the host (bpg_test_prover_stub_commitments)."""
    def __init__(self, ctx, transcript):
        super().__init__(None, transcript)
        self.test_stub_commitments()


class Case:
    def __init__(self, prover, transcript, commitments, inputs, gens_capacity, replay=None, label=None):
        self.prover, self.transcript, self.commitments, self.inputs, self.gens_capacity, self.replay = prover, transcript, commitments, inputs, gens_capacity, replay
        self.label = label                                  # the transcript label: what a verifier starts from


class Public:
    """the public values of one assembly: named as inputs (prover.input / verifier.input) or baked in as constants"""
    def __init__(self, cs, as_inputs):
        self.cs, self.as_inputs, self.values = cs, as_inputs, []

    def __call__(self, value: bytes):
        self.values.append(value)
        return bpg.LinearCombination.of(self.cs.input(value)) if self.as_inputs else bpg.LinearCombination.of(value)


# ------------------------------------------------------------------------------------------------ reference gadgets with the public side as inputs
def less_than(ctx, left: int, bound: int, as_inputs, tag="lt", prover_cls=bpg.Prover, delta=None):
    """LESS left < bound with the bound PUBLIC: n = 379, N = 512, m = 3 (left, delta, delta^-1).  delta: commit to another delta than bound - left (a
    witness that breaks the row (right - left) - delta)"""
    t = bpg.Transcript(b"LessThan"); p = prover_cls(ctx, t)
    pub = Public(p, as_inputs)
    ls = sc(left)
    lcom, lvar = p.commit(ls, blind(tag, 0))
    g = bpg.LessThan(lvar, ls, pub(sc(bound)), sc(bound))
    if delta is None:
        dcoms, derived = g.setup(p, [], [blind(tag, 1), blind(tag, 2)])
    else:
        d = [sc(delta), sc(pow(delta, L - 2, L))]
        dcoms, dvars = p.commit_many(d, [blind(tag, 1), blind(tag, 2)])
        derived = list(zip(d, dvars))
    g.prove(p, [], derived)

    def replay(v, bound_=bound, as_inputs_=False):
        vs = bpg.verifier_commit(v, [lcom] + dcoms)
        bpg.LessThan(vs[0], None, Public(v, as_inputs_)(sc(bound_)), None).verify(v, [], vs[1:])
    return Case(p, t, [lcom] + dcoms, pub.values, 512, replay, b"LessThan")


def inequality(ctx, left: int, right: int, as_inputs, tag="ne", prover_cls=bpg.Prover):
    """UNEQUAL left != right over one limb with the right-hand side PUBLIC: n = 3, m = 4 (left, delta, delta^-1, sum^-1)"""
    t = bpg.Transcript(b"Inequality"); p = prover_cls(ctx, t)
    pub = Public(p, as_inputs)
    ls = sc(left)
    lcom, lvar = p.commit(ls, blind(tag, 0))
    g = bpg.Inequality([pub(sc(right))], [sc(right)])
    dcoms, derived = g.setup(p, [ls], [blind(tag, 1 + i) for i in range(3)])
    g.prove(p, [lvar], derived)

    def replay(v, right_=right):
        vs = bpg.verifier_commit(v, [lcom] + dcoms)
        bpg.Inequality([bpg.LinearCombination.of(sc(right_))], None).verify(v, vs[:1], vs[1:])
    return Case(p, t, [lcom] + dcoms, pub.values, 4, replay, b"Inequality")


def set_membership(ctx, value: int, elements, as_inputs, tag="set", prover_cls=bpg.Prover):
    """SET value in {4 PUBLIC elements}: n = 8, m = 5 (value and the one-hot selector)"""
    t = bpg.Transcript(b"SetMembership"); p = prover_cls(ctx, t)
    pub = Public(p, as_inputs)
    vs_ = sc(value)
    vcom, vvar = p.commit(vs_, blind(tag, 0))
    es = [sc(e) for e in elements]
    g = bpg.SetMembership(vvar, vs_, [pub(e) for e in es], es)
    dcoms, derived = g.setup(p, [], [blind(tag, 1 + i) for i in range(len(es))])
    g.prove(p, [], derived)

    def replay(v, elements_=tuple(elements)):
        vs = bpg.verifier_commit(v, [vcom] + dcoms)
        bpg.SetMembership(vs[0], None, [bpg.LinearCombination.of(sc(e)) for e in elements_], None).verify(v, [], vs[1:])
    return Case(p, t, [vcom] + dcoms, pub.values, 8, replay, b"SetMembership")


def merkle_root(leaves):
    """the MiMC node hash of two leaves, read off an assembly-only prover over instance leaves (the sponge is the gadget's own)"""
    probe = bpg.Prover(None, bpg.Transcript(b"probe"))
    bpg.MerkleTree256(bytes(32), list(leaves), [], "(I I)").prove(probe, [], [])
    return probe.instance().aO[-32:]


def merkle_wi(ctx, leaf: int, sibling: int, as_inputs, tag="wi", prover_cls=bpg.Prover):
    """MERKLE root (W I): a committed leaf, its sibling and the root PUBLIC: n = 1944, N = 2048, m = 1.  Inputs: the sibling (inside the sponge's
    multiplications), then the root (a plain constrain() row)"""
    t = bpg.Transcript(b"MerkleTree"); p = prover_cls(ctx, t)
    pub = Public(p, as_inputs)
    ws, ss = sc(leaf), sc(sibling)
    root = merkle_root([ws, ss])
    wcom, wvar = p.commit(ws, blind(tag, 0))
    sib = pub(ss)
    bpg.MerkleTree256(pub(root), [sib], [bpg.LinearCombination.of(wvar)], "(W I)").prove(p, [], [])

    def replay(v, sibling_=sibling, root_=root):
        vs = bpg.verifier_commit(v, [wcom])
        bpg.MerkleTree256(root_, [sc(sibling_)], [bpg.LinearCombination.of(vs[0])], "(W I)").verify(v, [], [])
    c = Case(p, t, [wcom], pub.values, 2048, replay, b"MerkleTree")
    c.root = root
    return c


# name -> (builder, three (witness, public) argument tuples: one template, assigned to the other two)
GADGETS = {
    "set4": (set_membership, [(7, (3, 7, 11, 2**200 + 5)), (2**200 + 5, (3, 7, 11, 2**200 + 5)), (9, (9, L - 1, 0, 2**252 + 1))]),
    "inequality": (inequality, [(10, 3), (3, 10), (2**130 + 7, 2**130 + 6)]),            # left above, below, and one apart at a larger limb
    "less_than": (less_than, [(5, 1000), (2**125 - 3, 2**126 - 1), (0, 1)]),
    "merkle_wi": (merkle_wi, [(11, 22), (2**251 + 9, 5), (33, L - 1)]),
}


def build(name, k, as_inputs, ctx=None, prover_cls=bpg.Prover):
    fn, args = GADGETS[name]
    return fn(ctx, *args[k], as_inputs, tag="%s-%d" % (name, k), prover_cls=prover_cls)
