"""K statements against K different public values in ONE prover, for the tests of public inputs through repeat and join
(tests/test_template_repeat_inputs_host.py, tests/test_template_repeat_inputs_gpu.py).

The yardstick of both files is `assemble(parts, as_inputs=False)`: ONE prover that runs the gadget code item after item with every public value BAKED IN as a
constant (template_inputs_cases.Public(p, False)) - a host assembly that knows nothing of inputs, templates, repeats or joins.  A template is always made from
ONE item of another seed with as_inputs=True (`template_of`).  Seeds, blindings and values are pinned: nothing here is random at run time.

An item function appends one statement to a prover and returns (its commitments, the rows that are parameters, its checkpoint values); `ARGS[name][k]` are
the pinned arguments of item k of that gadget (k = 0 .. 7), `TEMPLATE_ARGS[name]` those of the template's own item."""
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import random_templates as RT
import template_inputs_cases as TC
from template_inputs_cases import Public, StubProver, sc, L


def blind(tag, i):
    return workloads.blinding("repeat-inputs-" + tag, i)


# ------------------------------------------------------------------------------------------------ the gadget codes, one item each
def inequality_item(p, pub, args, tag):
    left, right = args
    ls = sc(left)
    lcom, lvar = p.commit(ls, blind(tag, 0))
    g = bpg.Inequality([pub(sc(right))], [sc(right)])
    dcoms, derived = g.setup(p, [ls], [blind(tag, 1 + i) for i in range(3)])
    g.prove(p, [lvar], derived)
    return [lcom] + dcoms, [], []


def set4_item(p, pub, args, tag):
    value, elements = args
    vs = sc(value)
    vcom, vvar = p.commit(vs, blind(tag, 0))
    es = [sc(e) for e in elements]
    g = bpg.SetMembership(vvar, vs, [pub(e) for e in es], es)
    dcoms, derived = g.setup(p, [], [blind(tag, 1 + i) for i in range(len(es))])
    g.prove(p, [], derived)
    return [vcom] + dcoms, [], []


def less_than_item(p, pub, args, tag):
    """args = (left, bound) or (left, bound, delta): delta commits to another delta than bound - left (a witness that breaks the LAST row alone)"""
    left, bound = args[:2]
    ls = sc(left)
    lcom, lvar = p.commit(ls, blind(tag, 0))
    g = bpg.LessThan(lvar, ls, pub(sc(bound)), sc(bound))
    if len(args) < 3:
        dcoms, derived = g.setup(p, [], [blind(tag, 1), blind(tag, 2)])
    else:
        d = [sc(args[2]), sc(pow(args[2], L - 2, L))]
        dcoms, dvars = p.commit_many(d, [blind(tag, 1), blind(tag, 2)])
        derived = list(zip(d, dvars))
    g.prove(p, [], derived)
    return [lcom] + dcoms, [], []


def merkle_wi_item(p, pub, args, tag):
    """(W I): a committed leaf; the sibling (inside the sponge's products) and the root (a constrain() row) public.  Its one checkpoint is the node's digest."""
    leaf, sibling = args
    ws, ss = sc(leaf), sc(sibling)
    root = TC.merkle_root([ws, ss])
    wcom, wvar = p.commit(ws, blind(tag, 0))
    sib = pub(ss)
    bpg.MerkleTree256(pub(root), [sib], [bpg.LinearCombination.of(wvar)], "(W I)").prove(p, [], [])
    return [wcom], [], [root]


def random_item(seed, public=True):
    """a shape of random_templates: of the family with public inputs, or (public=False) of the family without any"""
    def item(p, pub, value_seed, tag):
        it = RT.item(p, seed, value_seed, public=pub if public else None, blind_tag="repeat-inputs-" + tag)
        item.last = it
        return [], it.rows, []
    item.seed = seed
    return item


ITEMS = {"inequality": (inequality_item, b"Inequality"), "set4": (set4_item, b"SetMembership"), "less_than": (less_than_item, b"LessThan"),
         "merkle_wi": (merkle_wi_item, b"MerkleTree")}
ARGS = {
    "inequality": [(10, 3), (3, 10), (2**130 + 7, 2**130 + 6), (0, L - 1), (5, 6), (7, 2**64), (1, 0), (2**252, 1)],
    "set4": [(7, (3, 7, 11, 2**200 + 5)), (2**200 + 5, (3, 7, 11, 2**200 + 5)), (9, (9, L - 1, 0, 2**252 + 1)), (0, (1, 2, 0, 3)), (4, (4, 4, 4, 4)),
             (L - 1, (5, L - 1, 6, 7)), (12, (13, 14, 15, 12)), (2, (2, 3, 5, 7))],
    "less_than": [(5, 1000), (2**125 - 3, 2**126 - 1), (0, 1), (8, 9), (2**64, 2**64 + 1), (77, 5000), (999, 1000), (1, 2**100)],
    "merkle_wi": [(11, 22), (2**251 + 9, 5), (33, L - 1), (1, 2), (3, 4), (5, 6), (7, 8), (9, 10)],
}
TEMPLATE_ARGS = {"inequality": (1234, 99), "set4": (21, (20, 21, 22, 23)), "less_than": (1, 2), "merkle_wi": (2**100, 2**200)}
GENS = {"inequality": 4, "set4": 8, "less_than": 512, "merkle_wi": 2048}

# Random shapes of the public=True family (random_templates.shape), chosen on the CPU for a property each; `shape_properties` recomputes it from the template's
# instance, and the host test asserts it per seed so that a change of the generator cannot silently drop the case.
#   three_ranges: parameter rows AND inputs in rows over a shared table (n = 8, m = 4, 3 inputs, 2 slots)      two_slots_one_input: one input under two different
#   coefficients (n = 5)      one_slot_two_rows: the same (input, coefficient) pair in two rows (n = 1, m = 5)      operands_only: inputs that no row names - hint
#   sources and zero coefficients only - so n_slots = 0 with n_inputs = 2 (n = 5, two parameter rows)
RANDOM_SEEDS = {"three_ranges": 1, "two_slots_one_input": 4, "one_slot_two_rows": 19, "operands_only": 49}


def item_fn(name):
    """name: a gadget of ITEMS, ("random", shape seed) or ("plain", shape seed): a random shape with / without public inputs"""
    if isinstance(name, tuple):
        return random_item(name[1], name[0] == "random"), b"random-template"
    return ITEMS[name]


class Assembly:
    """ONE prover over the items of `parts` = [(name, [args per item])], part after part: the prover, its transcript, the commitments, the public values in
    input order (part-major, item-major), the parameter rows with the constants assign() takes for them, the checkpoint values, per part the layout dims"""
    def __init__(self, parts, as_inputs, prover_cls=StubProver, ctx=None, label=None, tag="items"):
        names = [n for n, _ in parts]
        self.label = label or (item_fn(names[0])[1] if len(set(names)) == 1 else b"joined statement")
        self.transcript = bpg.Transcript(self.label)
        self.prover = p = prover_cls(ctx, self.transcript)
        self.pub = Public(p, as_inputs)
        self.commitments, self.rows, self.params, self.ck_values, self.items = [], [], [], [], []
        commit = p.commit

        def recording_commit(v, blinding):                   # random_templates.item keeps the variables and drops the commitments: keep them here
            com, var = commit(v, blinding)
            recorded.append(com)
            return com, var
        for pi, (name, args) in enumerate(parts):
            fn, _ = item_fn(name)
            for k, a in enumerate(args):
                recorded = []
                p.commit = recording_commit if isinstance(name, tuple) else commit
                coms, rows, cks = fn(p, self.pub, a,"%s-%s-%d-%d" % (tag, name if isinstance(name, str) else "%s%d" % name, pi, k))
                self.commitments += coms + recorded; self.rows += rows; self.ck_values += cks
                if isinstance(name, tuple):
                    self.params += fn.last.params
                    self.items.append(fn.last)
        self.inputs = list(self.pub.values)

    def instance(self):
        return self.prover.instance()


def replay(parts, commitments):
    """the VERIFIER's assembly of the same statement, public values as constants (gadget parts only) -> bpg.Verifier ready for its instance() / state"""
    LC = bpg.LinearCombination.of
    names = [n for n, _ in parts]
    v = bpg.Verifier(bpg.Transcript(ITEMS[names[0]][1] if len(set(names)) == 1 else b"joined statement"))
    at = 0
    for name, args in parts:
        for a in args:
            m = {"inequality": 4, "set4": 5, "less_than": 3, "merkle_wi": 1}[name]
            vs = bpg.verifier_commit(v, commitments[at:at + m])
            at += m
            if name == "inequality":
                bpg.Inequality([LC(sc(a[1]))], None).verify(v, vs[:1], vs[1:])
            elif name == "set4":
                bpg.SetMembership(vs[0], None, [LC(sc(e)) for e in a[1]], None).verify(v, [], vs[1:])
            elif name == "less_than":
                bpg.LessThan(vs[0], None, LC(sc(a[1])), None).verify(v, [], vs[1:])
            else:
                bpg.MerkleTree256(TC.merkle_root([sc(a[0]), sc(a[1])]), [sc(a[1])], [LC(vs[0])], "(W I)").verify(v, [], [])
    return v


def template_of(name, prover_cls=StubProver, ctx=None):
    """the gadget code assembled ONCE with as_inputs=True, from an item no test assigns -> Assembly"""
    args = 1000 + name[1] if isinstance(name, tuple) else TEMPLATE_ARGS[name]
    return Assembly([(name, [args])], True, prover_cls=prover_cls, ctx=ctx, tag="tmpl")


def template_parts(a):
    """(instance with its input terms, program with its parameter rows, hints, checkpoint variables, n_inputs) of a template's Assembly"""
    inst, values = a.prover.template_instance()
    prog, hints = a.prover.witness_program(hints=True)
    prog.param_rows = prog.param_rows + [r for r in a.rows if r not in prog.param_rows]
    cks = [v for v, _, last in a.prover.noted() if last] if a.ck_values else []
    return inst, prog, hints, cks, len(values)


def input_pairs(inst):
    """the (input, coefficient index) pairs of the template's rows in order of first appearance - its derived slots - and per pair the rows that name it"""
    pairs, rows = [], {}
    for r in range(inst.q):
        for t in range(int(inst.row_ptr[r]), int(inst.row_ptr[r + 1])):
            var = int(inst.term_var[t])
            if var >> 29 == bpg.VAR_INPUT:
                key = (var & 0x1fffffff, int(inst.term_coef[t]))
                if key not in rows:
                    pairs.append(key)
                rows.setdefault(key, set()).add(r)
    return pairs, rows


def shape_properties(a):
    """of a random template's Assembly: which of the four pinned properties hold"""
    inst, prog, _, _, n_in = template_parts(a)
    pairs, rows = input_pairs(inst)
    coefs_of = {}
    for p, ci in pairs:
        coefs_of.setdefault(p, set()).add(inst.coef[32 * ci:32 * ci + 32])
    return {"three_ranges": bool(prog.param_rows) and bool(pairs) and inst.ncoef > 0,
            "two_slots_one_input": any(len(c) > 1 for c in coefs_of.values()),
            "one_slot_two_rows": any(len(r) > 1 for r in rows.values()),
            "operands_only": n_in > 0 and not pairs}
