"""Assemblies for the tests of gated variables (Prover.gate): a hand-made circuit that meets every way a gated term is read, and Merkle paths - the GATED
path circuit (MerklePath256: one circuit for every leaf index, the index in its public inputs) beside the yardstick, a fresh host assembly of the reference
gadget MerkleTree256 with that index's pattern and the siblings baked in as instance values, which knows nothing of inputs or gates."""
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
from template_inputs_cases import StubProver, Case, Public, sc, L, merkle_root

LC = bpg.LinearCombination
PATH_LABEL = b"MerklePath"


def blind(tag, i):
    return workloads.blinding("gates-" + tag, i)


# ------------------------------------------------------------------------------------------------ the hand-made circuit
HAND_INPUTS = [(0, 1, L - 1, 2**252 + 9), (1, 0, 5, 7), (2**252 + 9, L - 1, 0, 1), (3, 11, 2**200 + 1, L - 2)]
HAND_VALUES = [(3, 4), (2**200 + 1, L - 2), (0, 9), (6, 2**130 + 5)]
HAND_N = 10


def hand10(inputs, values, gated, prover_cls=StubProver, ctx=None, tag="hand10"):
    """10 multipliers.  gated=True: the public values are inputs and the products input * variable are gates; gated=False: the same statement with the
    values baked in as constants, coefficient by coefficient (the yardstick).  A gate over a committed value; over the previous multiplier's output; over
    a_L of an earlier segment; under +1, -1 and a general coefficient; one variable gated by two inputs in one list; a gated term that shares its (input,
    coefficient) pair with a constant input term; a gate in a plain constrain() row; a gate as the source of a hint run; a gate over a variable the tests
    checkpoint (m3's output, HAND_CHECKPOINT)."""
    t = bpg.Transcript(b"hand10"); p = prover_cls(ctx, t)
    coms, vs = [], []
    for k, x in enumerate(values):
        com, var = p.commit(sc(x), blind(tag, k))
        coms.append(com); vs.append(var)
    if gated:
        X = [p.input(sc(x)) for x in inputs]
        G = lambda k, var, c=1: LC.of(p.gate(X[k], var)) * sc(c)
        K = lambda k, c=1: LC.of(X[k]) * sc(c)
    else:
        G = lambda k, var, c=1: LC.of(var) * sc(c * inputs[k] % L)
        K = lambda k, c=1: LC.of(sc(c * inputs[k] % L))
    m0 = p.multiply(G(0, vs[0]) + LC.of(vs[1]), LC.of(vs[0]) + K(1))                      # a committed value under +1
    m1 = p.multiply(G(1, m0[2], L - 1) + LC.of(1), LC.of(m0[0]))                           # the previous output (registers) under -1
    m2 = p.multiply(G(2, m1[2], 5) + G(3, m1[2], 7), LC.of(vs[1]) + LC.of(m1[1]))          # one variable, two inputs, general coefficients
    m3 = p.multiply(LC.of(vs[0]) + K(2, 5), G(2, vs[1], 5) + LC.of(m2[2]))                 # the pair (input 2, 5): a constant term and a gated term
    m4 = p.multiply(G(0, m0[0], 2**130) + LC.of(vs[0]), G(3, m3[2]) + LC.of(3))            # a_L of an earlier segment; m3's output (checkpointed)
    src = G(3, m3[2]) + LC.of(vs[1])
    src_value = (inputs[3] * _value(p, m3[2], gated) + values[1]) % L
    for bit in range(4):
        p.allocate_bit(src, bit, sc(src_value))                                            # m5..m8: a hint run whose source holds a gate
    m9 = p.multiply(G(2, m4[1]) + LC.of(m3[2]), LC.of(m4[2]) + K(0, L - 1))
    p.constrain(G(2, m4[1], 9) + LC.of(m3[2]) * sc(9) - LC.of(m9[0]) * sc(9))             # a plain row: 9 times what defines m9's left value
    return Case(p, t, coms, [sc(x) for x in inputs] if gated else [], 16)


HAND_CHECKPOINT = bpg.Variable(bpg.VAR_MULTIPLIER_OUTPUT << 29 | 3)


def _value(p, var, gated):
    """the value the prover assigned to a multiplier variable so far"""
    inst = p.template_instance()[0] if gated else p.instance()
    vec = (inst.aL, inst.aR, inst.aO)[int(var) >> 29]
    i = int(var) & 0x1fffffff
    return int.from_bytes(vec[32 * i:32 * i + 32], "little")


# ------------------------------------------------------------------------------------------------ Merkle paths
def host_tree(leaves):
    """levels of the MiMC tree over `leaves` (32-byte scalars, a power of two of them), leaves first, the root last - hashed by the gadget's own sponge"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([merkle_root([cur[i], cur[i + 1]]) for i in range(0, len(cur), 2)])
    return levels


def host_path(levels, index):
    """(siblings bottom up, nodes on the path from the leaf's parent to the root) - MerkleTree.paths / MerkleTree.path_nodes on the host"""
    sib, nodes = [], []
    for j in range(len(levels) - 1):
        sib.append(levels[j][(index >> j) ^ 1])
        nodes.append(levels[j + 1][index >> (j + 1)])
    return sib, nodes


def reference_pattern(index, depth):
    """the pattern of leaf `index`'s path with a witness leaf and instance siblings, and the order in which the gadget consumes the siblings"""
    pat, order = "W", []
    for k in range(depth):
        if (index >> k) & 1:
            pat, order = workloads.hash_pattern("I", pat), [k] + order
        else:
            pat, order = workloads.hash_pattern(pat, "I"), order + [k]
    return pat, order


def path_reference(ctx, index, leaf, siblings, root, prover_cls=StubProver, tag="path"):
    """the yardstick: MerkleTree256 over the index's pattern, siblings and root as constants"""
    t = bpg.Transcript(PATH_LABEL); p = prover_cls(ctx, t)
    com, var = p.commit(leaf, blind(tag, 0))
    pat, order = reference_pattern(index, len(siblings))
    bpg.MerkleTree256(root, [siblings[k] for k in order], [LC.of(var)], pat).prove(p, [], [])
    return Case(p, t, [com], [], _pow2(p.get_num_multiplications()))


def path_gated(ctx, index, leaf, siblings, root, prover_cls=StubProver, tag="path"):
    """MerklePath256: 4 inputs per level and the root, their values from merkle_path_inputs"""
    t = bpg.Transcript(PATH_LABEL); p = prover_cls(ctx, t)
    com, var = p.commit(leaf, blind(tag, 0))
    values = bpg.merkle_path_inputs(index, siblings, root)
    xs = [p.input(v) for v in values]
    d = len(siblings)
    bpg.MerklePath256(xs[4 * d], var, [tuple(xs[4 * j:4 * j + 4]) for j in range(d)]).prove(p, [], [])
    return Case(p, t, [com], values, _pow2(p.get_num_multiplications()))


def path_verifier(commitment, values):
    """the verifier's assembly of the gated path for these input values -> (transcript, verifier)"""
    t = bpg.Transcript(PATH_LABEL); v = bpg.Verifier(t)
    var = v.commit(commitment)
    xs = [v.input(x) for x in values]
    d = (len(values) - 1) // 4
    bpg.MerklePath256(xs[4 * d], var, [tuple(xs[4 * j:4 * j + 4]) for j in range(d)]).verify(v, [], [])
    return t, v


def node_checkpoints(prover):
    """the node hashes of a path circuit as checkpoint variables, bottom up (the digests the sponge notes): their values are MerkleTree.path_nodes"""
    return [var for var, _, last in prover.noted() if last]


def _pow2(n):
    cap = 1
    while cap < n:
        cap *= 2
    return cap


def sample_leaves(count, tag="leaves"):
    return [sc(int.from_bytes(workloads.synth("gates-" + tag, i, 31), "little")) for i in range(count)]
