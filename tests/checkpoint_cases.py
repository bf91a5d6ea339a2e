"""The circuits of the checkpoint tests (test_template_checkpoints_host.py, test_template_checkpoints_gpu.py), each with the checkpoint VALUES computed
without the circuit: Python integers for the hand-built chain, the native host sponge (bpg.mimc_sponge, bpg.mimc_sponge_states) for the hash circuits.

Every builder returns a workloads.Assembled with
    ck_vars    the checkpointed Variables, in the order their values are given
    ck_values  their 32-byte values
so that `prover.template(ctx, param_rows=[last row], checkpoints=a.ck_vars)` made from one seed can be assigned the values of another."""
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads

L = bpg.L
sc = lambda x: (x % L).to_bytes(32, "little")
LC = bpg.LinearCombination

CHAIN_BLOCKS, CHAIN_ROUNDS = 6, 3


def chain_constant(k, r):
    return 7 + 3 * k + r


def chain(ctx, seed=0, prover_cls=bpg.Prover, items=1):
    """six blocks of three rounds t = x + v_k + c; x = (t * t) * t, one committed value per block; x starts at 0; closing constraint x - digest = 0.
    n = 36, q = 73.  Checkpoints: the output of blocks 0..4 (what links one block to the next).
    items > 1: the same gadget code `items` times in ONE prover, item by item (commitments, then multipliers, then the closing constraint) - the circuit
    ResidentCircuit.repeat(items) makes on the device; ck_vars are item 0's, ck_values item-major, param_rows one per item."""
    cfg = "ck-chain-%d" % seed
    t = bpg.Transcript(b"CheckpointChain")
    p = prover_cls(ctx, t)
    coms, ck_vars, ck_values, rows = [], [], [], []
    for item in range(items):
        vals = [int.from_bytes(workloads.synth(cfg, CHAIN_BLOCKS * item + k, 31), "little") for k in range(CHAIN_BLOCKS)]
        c, vs = p.commit_many([sc(v) for v in vals], [workloads.blinding(cfg, CHAIN_BLOCKS * item + k) for k in range(CHAIN_BLOCKS)])
        coms += c
        x_lc, x, links, states = LC.of(0), 0, [], []
        for k in range(CHAIN_BLOCKS):
            for r in range(CHAIN_ROUNDS):
                t_lc = x_lc + vs[k] + chain_constant(k, r)
                sq = p.multiply(t_lc, t_lc)
                cube = p.multiply(LC.of(sq[2]), LC.of(sq[0]))
                x_lc = LC.of(cube[2])
                x = pow(x + vals[k] + chain_constant(k, r), 3, L)
            links.append(cube[2]); states.append(sc(x))
        p.constrain(x_lc - sc(x))
        rows.append(p.num_constraints() - 1)
        if item == 0:
            ck_vars = links[:-1]
        ck_values += states[:-1]
    cap = 64
    while cap < p.get_num_multiplications():
        cap *= 2
    a = workloads.Assembled(p, t, coms, cap, None)
    a.ck_vars, a.ck_values, a.param_rows = ck_vars, ck_values, rows
    return a


def preimage3(ctx, seed=0, prover_cls=bpg.Prover):
    """MimcHash256 over an 80-byte preimage: two full blocks and the padded last one, n = 3 * 972 = 2,916, m = 5 (three blocks, the padded block, the
    padding).  Checkpoints: every note (the state after each absorbed block; the third is the digest)."""
    a = workloads.mimc_preimage(ctx, nbytes=80, seed=seed, prover_cls=prover_cls)
    v = a.prover.instance().v
    blocks = [v[0:32], v[32:64], v[96:128]]                  # the sponge absorbs the first two blocks and the PADDED last one (committed value 3)
    a.ck_vars = [var for var, _, _ in a.prover.noted()]
    a.ck_values = bpg.mimc_sponge_states(blocks)
    a.gens_capacity = 4096
    return a


def host_tree(leaves):
    """levels[0] = the leaves, levels[d] = [root]: node = mimc_sponge([left, right])"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        lo = levels[-1]
        levels.append([bpg.mimc_sponge([lo[i], lo[i + 1]]) for i in range(0, len(lo), 2)])
    return levels


def tree_leaves(seed, count):
    return [b"\x07" + workloads.synth("ck-tree-%d" % seed, i, 31) for i in range(count)]      # big-endian, top byte small: canonical scalars


def path_values(levels, index, order):
    """the committed values of a path circuit in the order the gadget consumes them (workloads.merkle_path_pattern)"""
    return [levels[0][index] if what == "leaf" else levels[k][(index >> k) ^ 1] for what, k in order]


def path_nodes(levels, index):
    return [levels[k][index >> k] for k in range(1, len(levels))]


def path_from(ctx, levels, index, cfg, prover_cls=bpg.Prover):
    """the authentication path of leaf `index` of a tree given by its levels (little-endian scalars): n = depth * 1,944, m = depth + 1.
    Checkpoints: the digest of every node on the path (the is_last notes), bottom up, the root included."""
    depth = len(levels) - 1
    pattern, order = workloads.merkle_path_pattern(index, depth)
    values = path_values(levels, index, order)
    t = bpg.Transcript(b"MerklePath")
    p = prover_cls(ctx, t)
    coms, vs = p.commit_many(values, [workloads.blinding(cfg, i) for i in range(len(values))])
    bpg.MerkleTree256(levels[-1][0], [], bpg.vars_to_lc(vs), pattern).prove(p, [], [])
    cap = 1
    while cap < p.get_num_multiplications():
        cap *= 2
    a = workloads.Assembled(p, t, coms, cap, None)
    a.ck_vars = [var for var, _, last in p.noted() if last]
    a.ck_values = path_nodes(levels, index)
    a.values, a.root, a.order, a.pattern = values, levels[-1][0], order, pattern
    return a


def path(ctx, index, depth=3, seed=0, prover_cls=bpg.Prover):
    levels = host_tree([bpg.be_to_scalar(b) for b in tree_leaves(seed, 1 << depth)])
    return path_from(ctx, levels, index, "ck-path-%d-%d" % (seed, index), prover_cls)


def full_tree4(ctx, seed=1, prover_cls=bpg.Prover):
    """the depth-2 full tree ((W W)(W W)): n = 3 * 1,944.  Checkpoints: the three node digests in assembly order (left node, right node, root)."""
    a = workloads.merkle_full_tree(ctx, leaves=4, seed=seed, prover_cls=prover_cls)
    v = a.prover.instance().v
    levels = host_tree([v[32 * i:32 * i + 32] for i in range(4)])
    a.ck_vars = [var for var, _, last in a.prover.noted() if last]
    a.ck_values = [levels[1][0], levels[1][1], levels[2][0]]
    return a


def last_row(a):
    return a.prover.num_constraints() - 1


def constant_term(inst, row):
    """the constant term of a constraint row of a host-assembled instance (the sum of its One terms): what assign() is given for a parameter row"""
    a, b = int(inst.row_ptr[row]), int(inst.row_ptr[row + 1])
    s = sum(int.from_bytes(inst.coef[32 * int(inst.term_coef[k]):32 * int(inst.term_coef[k]) + 32], "little") for k in range(a, b) if int(inst.term_var[k]) >> 29 == 4)
    return sc(s)
